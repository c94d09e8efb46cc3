// cfs_hip.hip -- gfx950 (MI355X, CDNA4) kernels and the C ABI of libcfs_hip.so.
//
// The hot path of athelaf/cfs-spmv -- cpu_mv_sym_conflict_free_v2,
// include/matrix/csr_matrix.tpp:2965-3028: walk the strict lower triangle once,
// update both y_i (row side) and y_j (transposed side) -- as hand-written HIP
// for 64-lane wavefronts.  HBM-bandwidth bound (0.3 flop/byte): no MFMA.
// The schedule the kernels walk is built by cfs_plan.hpp.
//
// Written for gfx950 only; compile with hipcc --offload-arch=gfx950.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "cfs_hip.h"
#include "cfs_plan.hpp"
#include "cfs_planfile.hpp"
#include "cfs_runtime.hpp"
#include "cfs_comm.hpp"

using cfs_plan::SymPlan;
using cfs_plan::Tile;

// ---------------------------------------------------------------------------
// runtime (cfs_runtime.hpp): per-device contexts, pools, error plumbing
// ---------------------------------------------------------------------------
using cfs_rt::DevBuf;
using cfs_rt::DeviceGuard;
using cfs_rt::PinBuf;
using cfs_rt::set_err;

static int ensure_init() { return cfs_rt::ensure_home(); }

// copy with non-temporal stores (dst 16-byte aligned): a staging block is written once and read by the
// DMA engine, never by this CPU -- ordinary stores would first read every destination line into the cache
// (read-for-ownership: three memory transfers per byte instead of two; glibc only switches to streaming
// stores for copies far larger than one thread's 1 MiB share of a piece)
static void stream_copy(char *dst, const char *src, size_t n) {
  typedef long long v2 __attribute__((vector_size(16), aligned(16)));
  typedef long long v2u __attribute__((vector_size(16), aligned(1)));
  if (((uintptr_t)dst & 15) != 0) {
    memcpy(dst, src, n);
    return;
  }
  size_t i = 0;
  for (; i + 64 <= n; i += 64) {
    const v2u a = *reinterpret_cast<const v2u *>(src + i), b = *reinterpret_cast<const v2u *>(src + i + 16),
              c = *reinterpret_cast<const v2u *>(src + i + 32), d = *reinterpret_cast<const v2u *>(src + i + 48);
    __builtin_nontemporal_store((v2)a, reinterpret_cast<v2 *>(dst + i));
    __builtin_nontemporal_store((v2)b, reinterpret_cast<v2 *>(dst + i + 16));
    __builtin_nontemporal_store((v2)c, reinterpret_cast<v2 *>(dst + i + 32));
    __builtin_nontemporal_store((v2)d, reinterpret_cast<v2 *>(dst + i + 48));
  }
  if (i < n) memcpy(dst + i, src + i, n - i);
  __builtin_ia32_sfence();
}
void cfs_rt::parallel_copy(void *dst, const void *src, size_t bytes) {
  const int T = cfs_plan::host_threads();
  static const bool stream = !(getenv("CFS_HIP_STREAM_COPY") && atoi(getenv("CFS_HIP_STREAM_COPY")) == 0);
  if (bytes < ((size_t)1 << 20) || T < 2) {
    memcpy(dst, src, bytes);
    return;
  }
  const size_t chunk = ((bytes + T - 1) / T + 4095) & ~(size_t)4095;
#pragma omp parallel for schedule(static) num_threads(T)
  for (int t = 0; t < T; t++) {
    const size_t b = (size_t)t * chunk;
    if (b >= bytes) continue;
    const size_t len = std::min(chunk, bytes - b);
    if (stream) stream_copy((char *)dst + b, (const char *)src + b, len);
    else memcpy((char *)dst + b, (const char *)src + b, len);
  }
}

// ---------------------------------------------------------------------------
// device view of a plan
// ---------------------------------------------------------------------------
template <typename V> struct SymDev {
  const Tile *tiles;
  const Tile *gfirst;
  const int2 *group_range; // per launch slot: [first, last) tile
  const int32_t *slot_col; // original column of every slot of every tile
  const uint32_t *rowinfo;
  const V *diag;
  const uint4 *slice_meta; // {value offset, slot offset | lanes of packet 0 << 25, leader mask}
  const uint8_t *leadlane; // per slice and lane: the lane whose slots it reads
  const V *vals;
  const uint16_t *slots;
  const V *cvals; // COO leftovers (len % 4 per row): value, row slot, column slot
  const uint16_t *crows;
  const uint16_t *ccols;
  const V *fvals; // FAR sections (HYB): value, own row slot, global column
  const uint16_t *frows;
  const int32_t *fcols;
  V *strip;
  int row_begin;
  int lds_slots;
};

// one packet = 4 consecutive entries of the rows held by lanes [0, cnt): values
// for lane l, entry j at cfs_plan::packet_val_pos<V>(l, j, cnt), slots at l*4+j.
// Every lane issues the loads (lanes >= cnt re-read lane cnt-1's bytes: same
// cache lines, no extra DRAM traffic) so that the loads are unconditional
// instructions and the compiler's vmcnt bookkeeping stays exact.
template <typename V> struct Pkt {
  V v[4];
  ushort4 c;
};

// `leaders` (one bit per lane of the slice): a lane whose slot sequence is a
// prefix of an earlier lane's stores no slots and reads that LEADER lane's
// (cfs_plan::SymPlan::leadlane, one byte per lane).  A leader's block inside a
// packet's slot block is its rank among the leaders: lanes are sorted by packet
// count, so every leader below it is active whenever it is.
__device__ __forceinline__ int leader_rank(unsigned long long leaders, int leader_lane) {
  return __popcll(leaders & ((1ull << leader_lane) - 1ull));
}
// leaders among the cnt active lanes of a packet
__device__ __forceinline__ int active_leaders(unsigned long long leaders, int cnt) {
  return cnt > 0 ? __popcll(leaders & (~0ull >> (64 - cnt))) : 0;
}
// A matrix stream larger than the 256 MiB Infinity Cache is read exactly once
// per SpMV: its loads then carry the non-temporal hint (NT) so that they do not
// displace x, y, the slot tables and the strips from L2 / Infinity Cache
// (measured: Flan stand-in 0.117 -> 0.110 ms).  A stream that FITS the cache
// (ldoor, pwtk stand-ins) is served from it on every SpMV after the first and
// must stay cacheable (ldoor: 0.049 ms plain vs 0.057 ms with NT).
typedef double cfs_d2 __attribute__((ext_vector_type(2)));
typedef float cfs_f4 __attribute__((ext_vector_type(4)));
typedef unsigned short cfs_us4 __attribute__((ext_vector_type(4)));
template <bool NT, typename T> __device__ __forceinline__ T stream_load(const T *p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}
// lrank = rank of this lane's leader; a lane past the packet's end is clamped to
// the last stored block (same cache lines, bytes unused)
template <bool NT>
__device__ __forceinline__ void fetch_packet(Pkt<double> &p, const double *tv,
                                             const uint16_t *ts, uint32_t off, uint32_t soff,
                                             int cnt, unsigned long long leaders, int lane,
                                             int lrank) {
  const int ll = min(lane, max(cnt, 1) - 1);
  const int rk = min(lrank, max(active_leaders(leaders, cnt), 1) - 1);
  const cfs_d2 lo = stream_load<NT>(reinterpret_cast<const cfs_d2 *>(tv + off + ll * 2));
  const cfs_d2 hi = stream_load<NT>(reinterpret_cast<const cfs_d2 *>(tv + off + 2 * cnt + ll * 2));
  const cfs_us4 c = stream_load<NT>(reinterpret_cast<const cfs_us4 *>(ts + soff + rk * 4));
  p.c = make_ushort4(c.x, c.y, c.z, c.w);
  p.v[0] = lo.x; p.v[1] = lo.y; p.v[2] = hi.x; p.v[3] = hi.y;
}
template <bool NT>
__device__ __forceinline__ void fetch_packet(Pkt<float> &p, const float *tv,
                                             const uint16_t *ts, uint32_t off, uint32_t soff,
                                             int cnt, unsigned long long leaders, int lane,
                                             int lrank) {
  const int ll = min(lane, max(cnt, 1) - 1);
  const int rk = min(lrank, max(active_leaders(leaders, cnt), 1) - 1);
  const cfs_f4 q = stream_load<NT>(reinterpret_cast<const cfs_f4 *>(tv + off + ll * 4));
  const cfs_us4 c = stream_load<NT>(reinterpret_cast<const cfs_us4 *>(ts + soff + rk * 4));
  p.c = make_ushort4(c.x, c.y, c.z, c.w);
  p.v[0] = q.x; p.v[1] = q.y; p.v[2] = q.z; p.v[3] = q.w;
}
// entries of the packet's slot block = 4 x (leaders among its cnt lanes)
__device__ __forceinline__ uint32_t slot_block(unsigned long long leaders, int cnt) {
  return 4u * (uint32_t)active_leaders(leaders, cnt);
}

// one stored nonzero a = A[row][col(c)]: row side into the register
// accumulator, transposed side into the LDS y window (ds_add_f64 / ds_add_f32)
//
// The y window is ALWAYS fp64: on gfx950 ds_add_f64 runs at the rate of the
// matrix stream while ds_add_f32 is ~4x slower under this access pattern
// (measured: fp32 tile kernel 0.370 ms with ds_add_f32 vs 0.084 ms without the
// transposed atomics), so the single-precision build accumulates the window in
// double and rounds once when the window is flushed.
// OFFB (a mirrored shard, cfs_plan::Options::mirror_offblock): slots >= ny are
// off-block columns; their entries are one-sided -- row side only, the rank that
// owns the column computes the transposed side from its own copy of the entry.
// The y window of a tile.  Default: one fp64 word per slot, ds_add_f64 -- the order in
// which the waves' updates of a slot arrive varies from run to run, and so do the last
// bits of y.  DETERMINISTIC (CFS_HIP_FLAG_DETERMINISTIC): every contribution p is
// turned into a fixed-point number of 2 x 40 bits below a PER-SLOT scale 2^e and added
// with INTEGER atomics (hi and lo word of the slot): integer addition is associative,
// so the sums -- and y -- are bit-identical whatever the order.  e = (exponent bound of
// the 1-norm of the slot's matrix row, cfs_plan: 2^ex > sum_j |a_ij|) + (exponent of
// the largest |x| in the tile's window): a bound of EVERY partial sum of the slot, so
// the hi word never needs more than 40 bits, and a contribution keeps 2^-80 of its
// own row's scale -- the precision does not depend on how the matrix is scaled
// (round 2 used one scale per tile: rows 2^-15 below the tile's largest lost bits).
template <bool DET> struct YWin {
  double *y;         // !DET: fp64 sums.  DET: the hi words (as long long)
  long long *lo;     // DET: the lo words
  const short *ex;   // DET: per slot, exponent bound of the row's 1-norm (LDS)
  int xe;            // DET: exponent of the window's largest |x| (|x| < 2^xe), wave-uniform
  __device__ __forceinline__ void add(unsigned slot, double p) const {
    if (!DET) {
      atomicAdd(&y[slot], p);
    } else {
      const double q = ldexp(p, 40 - ((int)ex[slot] + xe)); // exact: a power of two
      const double h = trunc(q);
      const long long hi = (long long)h;
      const long long l2 = (long long)rint((q - h) * 0x1p40); // q - h is exact
      atomicAdd(reinterpret_cast<unsigned long long *>(y) + slot, (unsigned long long)hi);
      atomicAdd(reinterpret_cast<unsigned long long *>(lo) + slot, (unsigned long long)l2);
    }
  }
  __device__ __forceinline__ void zero(unsigned slot) const {
    if (!DET) {
      y[slot] = 0.0;
    } else {
      reinterpret_cast<long long *>(y)[slot] = 0;
      lo[slot] = 0;
    }
  }
  // value of a slot; mul = 1, or NaN when the window of x held a NaN / Inf
  __device__ __forceinline__ double get(unsigned slot, double mul) const {
    if (!DET) return y[slot];
    const long long hi = reinterpret_cast<const long long *>(y)[slot];
    const int e = (int)ex[slot];
    // (a row that holds a NaN / Inf has no fixed-point image either: it reads NaN)
    if (e >= cfs_plan::kExpNonFinite) return __longlong_as_double(0x7ff8000000000000ll);
    return ldexp((double)hi + (double)lo[slot] * 0x1p-40, e + xe - 40) * mul;
  }
};
// 2^k as a double, k clamped to the normal range
__device__ __forceinline__ double pow2_double(int k) {
  k = max(-1000, min(1000, k));
  return __longlong_as_double((long long)(k + 1023) << 52);
}

template <typename V, int MODE, bool OFFB, bool DET>
__device__ __forceinline__ void lds_update(const V *xl, const YWin<DET> &yw, V a, unsigned c, V xi,
                                           V &acc, unsigned ny) {
  if (MODE == 2) {
    acc = fma(a, xi + V(c), acc);
  } else {
    acc = fma(a, xl[c], acc);
    if (MODE == 0 && (!OFFB || c < ny)) yw.add(c, (double)a * (double)xi);
  }
}
template <typename V, int MODE, bool OFFB, bool DET>
__device__ __forceinline__ void consume_packet(const Pkt<V> &p, const V *xl, const YWin<DET> &yl,
                                               V xi, V &acc, unsigned ny) {
  lds_update<V, MODE, OFFB, DET>(xl, yl, p.v[0], p.c.x, xi, acc, ny);
  lds_update<V, MODE, OFFB, DET>(xl, yl, p.v[1], p.c.y, xi, acc, ny);
  lds_update<V, MODE, OFFB, DET>(xl, yl, p.v[2], p.c.z, xi, acc, ny);
  lds_update<V, MODE, OFFB, DET>(xl, yl, p.v[3], p.c.w, xi, acc, ny);
}
// The lanes of one mesh node read the same slots, i.e. their transposed updates of one
// packet entry go to the SAME y-window word: one instruction, up to three lanes on one
// address.  A follower that sits right behind a lane of its group hands its product to
// that lane (two DPP row shifts, runs of at most three lanes; cfs_plan sets the flags)
// and only the head of a run issues the atomic: fewer active lanes, no same-address
// serialisation.  `give` = my products go to my left neighbour, `take` = I add my right
// neighbour's.  Inactive lanes contribute 0 (a follower never has more packets than
// the lane to its left: lanes are sorted by packet count).
__device__ __forceinline__ double row_shl1(double v) { // lane l <- lane l + 1 (0 at the end of a row of 16)
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x101, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x101, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <typename V, bool OFFB, bool DET>
__device__ __forceinline__ void entry_combined(const V *xl, const YWin<DET> &yw, V a, unsigned c, V xi,
                                               V &acc, unsigned ny, bool act, bool give, bool take) {
  double pr = 0.0;
  if (act) {
    acc = fma(a, xl[c], acc);
    pr = (double)a * (double)xi;
  }
  // (the shifts run with every lane enabled: a DPP read of a disabled lane returns nothing)
  const double t1 = row_shl1(pr);
  const double s1 = pr + (take ? t1 : 0.0);
  const double t2 = row_shl1(s1);
  const double q = pr + (take ? t2 : 0.0);
  if (act && !give && (!OFFB || c < ny)) yw.add(c, q);
}
template <typename V, bool OFFB, bool DET>
__device__ __forceinline__ void consume_combined(const Pkt<V> &p, const V *xl, const YWin<DET> &yl, V xi,
                                                 V &acc, unsigned ny, bool act, bool give, bool take) {
  entry_combined<V, OFFB, DET>(xl, yl, p.v[0], p.c.x, xi, acc, ny, act, give, take);
  entry_combined<V, OFFB, DET>(xl, yl, p.v[1], p.c.y, xi, acc, ny, act, give, take);
  entry_combined<V, OFFB, DET>(xl, yl, p.v[2], p.c.z, xi, acc, ny, act, give, take);
  entry_combined<V, OFFB, DET>(xl, yl, p.v[3], p.c.w, xi, acc, ny, act, give, take);
}
// one COO leftover a = A[row(r)][col(c)]: both sides through LDS atomics
template <typename V, int MODE, bool OFFB, bool DET>
__device__ __forceinline__ void coo_update(const V *xl, const YWin<DET> &yl, V a, unsigned r,
                                           unsigned c, unsigned ny) {
  if (MODE == 0 || MODE == 1) {
    yl.add(r, (double)a * (double)xl[c]);
    if (MODE == 0 && (!OFFB || c < ny)) yl.add(c, (double)a * (double)xl[r]);
  }
}

// ---------------------------------------------------------------------------
// tile kernel: persistent workgroups, each walks its group of tiles.
//   prologue: x window -> LDS (own rows coalesced, halo gathered), y window = 0
//   slices  : one lane = one row; row-side sum in a register, transposed
//             updates into the LDS y window with ds_add_f64 / ds_add_f32.
//             The matrix stream is software-pipelined per wave: the head
//             packet of the NEXT slice is requested a whole slice ahead and
//             packets ping-pong between two register sets, so a wave always
//             has loads in flight, also across slice boundaries.  The len%4
//             leftovers of the tile's rows are a flat COO section.
//   epilogue: own rows -> y (plain coalesced stores, fully overwrites y),
//             halo sums -> this tile's private strip (plain coalesced stores)
// MODE 0 is the product kernel.  MODE 1/2 are timing-only ablations selected by
// cfs_hip_options.flags (results are WRONG by construction; they exist to price
// the LDS atomics / LDS gathers against the pure matrix stream, never shipped
// as a result path): 1 = no transposed LDS atomics, 2 = no LDS traffic at all,
// 3 = windows only (no matrix stream), 4 = matrix stream only (no windows).
// ---------------------------------------------------------------------------
// (second launch bound: 4 waves per SIMD must stay resident -- two 512-thread
// workgroups, or one of 1 024, per CU -- i.e. at most 128 VGPRs; the persistent grid
// is sized for exactly that residency)
template <typename V, int BLOCK, int MODE, bool NT, bool OFFB, int U, bool DET = false, bool COMB = true>
__global__ void __launch_bounds__(BLOCK, 4)
    cfs_sym_tile_kernel(const Tile *__restrict__ a_tiles, const Tile *__restrict__ a_gfirst,
                        const int2 *__restrict__ a_group_range,
                        const int32_t *__restrict__ a_slot_col,
                        const uint32_t *__restrict__ a_rowinfo, const V *__restrict__ a_diag,
                        const uint4 *__restrict__ a_slice_meta,
                        const uint8_t *__restrict__ a_leadlane, const V *__restrict__ a_vals,
                        const uint16_t *__restrict__ a_slots, const V *__restrict__ a_cvals,
                        const uint16_t *__restrict__ a_crows,
                        const uint16_t *__restrict__ a_ccols, const V *__restrict__ a_fvals,
                        const uint16_t *__restrict__ a_frows, const int32_t *__restrict__ a_fcols,
                        V *__restrict__ a_strip, const int a_row_begin, const int a_lds_slots,
                        const V *__restrict__ x, V *__restrict__ y,
                        unsigned long long *__restrict__ dbg, const short *__restrict__ a_slot_exp) {
  // every array is a separate __restrict__ argument: read-only metadata at
  // wave-uniform addresses then becomes scalar loads (s_load), off the vector
  // memory counter the matrix stream is pipelined on
  struct {
    const Tile *__restrict__ tiles;
    const Tile *__restrict__ gfirst;
    const int2 *__restrict__ group_range;
    const int32_t *__restrict__ slot_col;
    const uint32_t *__restrict__ rowinfo;
    const V *__restrict__ diag;
    const uint4 *__restrict__ slice_meta;
    const uint8_t *__restrict__ leadlane;
    const V *__restrict__ vals;
    const uint16_t *__restrict__ slots;
    const V *__restrict__ cvals;
    const uint16_t *__restrict__ crows;
    const uint16_t *__restrict__ ccols;
    const V *__restrict__ fvals;
    const uint16_t *__restrict__ frows;
    const int32_t *__restrict__ fcols;
    V *__restrict__ strip;
    int row_begin, lds_slots;
  } d = {a_tiles, a_gfirst, a_group_range, a_slot_col, a_rowinfo, a_diag, a_slice_meta, a_leadlane, a_vals,
         a_slots, a_cvals, a_crows, a_ccols, a_fvals, a_frows, a_fcols, a_strip, a_row_begin, a_lds_slots};
  // slice ticket counter of the current tile (16 B so the dynamic region below
  // stays 16-byte aligned)
  __shared__ __align__(16) int cfs_ticket[4];
  extern __shared__ __align__(16) unsigned char cfs_smem[];
  // y window first (8-byte words: one per slot, two in the deterministic build), then x
  YWin<DET> yl;
  yl.y = reinterpret_cast<double *>(cfs_smem);
  yl.lo = reinterpret_cast<long long *>(cfs_smem) + (DET ? d.lds_slots : 0);
  V *xl = reinterpret_cast<V *>(yl.y + (DET ? 2 : 1) * d.lds_slots);
  short *exl = reinterpret_cast<short *>(xl + d.lds_slots); // DET: per-slot scale exponents
  yl.ex = exl;
  yl.xe = 0;
  if (DET) { // exponent of max |x| in the window: two words, tiles alternate
    if (threadIdx.x == 0) cfs_ticket[2] = cfs_ticket[3] = 0;
    __syncthreads();
  }
  int det_parity = 0;
  const int tid = threadIdx.x, lane = tid & 63;
  // wave-uniform by construction: keep it in an SGPR so that slice bookkeeping is
  // scalar (s_load / s_cbranch) and never waits on the vector-memory counter
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NW = BLOCK / 64;
  // blocks b and b+8 share an XCD (round-robin dispatch): give every XCD a
  // contiguous run of groups so neighbouring tiles share halo lines in one L2.
  // Placement only affects speed, never correctness.
  const int nper = gridDim.x >> 3;
  // (g is a launch SLOT: which group of the plan runs in it is the host's choice,
  // SymPlan::launch_order -- gfirst / group_range are stored in slot order)
  const int g = (blockIdx.x & 7) * nper + (blockIdx.x >> 3);
  const int2 trange = d.group_range[g];
  const int t0 = trange.x, t1 = trange.y;
  // developer timeline (cfs_hip_sym_debug_timeline): 100 MHz wall clock stamps of
  // this workgroup's phases; dbg is NULL in every product launch
  if (dbg && tid == 0) dbg[blockIdx.x * 8 + 0] = __builtin_amdgcn_s_memrealtime();

  // x window of a tile, gathered into registers with every load in flight at
  // once (two round trips: halo columns, then x).  Under a saturated memory
  // system a round trip costs microseconds, so the window of the NEXT tile is
  // requested before the barrier that ends the current tile's slices and lands
  // while the y window is flushed.
  // U = LDS slots one thread fills / flushes.  Every thread issues all U gathers
  // (clamped, unconditional), so a launch whose windows are small uses the
  // instantiation with the smallest U that covers them: a tile with 1 100 slots
  // would otherwise issue 78 % of its start-up loads for nothing.
  static_assert(U <= cfs_plan::kSlotsPerThread, "U");
  V xr[U];
  short er[DET ? U : 1]; // DET: the slots' scale exponents, fetched with the slot table
  bool first_gather = true;
  auto gather_x = [&](const Tile &tn) {
    // every load is unconditional (clamped index): a load under a divergent
    // branch would make the compiler drain vmcnt before the other side of the
    // branch may write the same register.  Own rows go through the slot table
    // too: tiles are clusters of the matrix graph, not runs of consecutive rows.
    int idx[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int i = min(tid + k * BLOCK, tn.nslots - 1);
      idx[k] = d.slot_col[tn.slot_off + i]; // slot_col is padded by one entry
      if (DET) er[k] = a_slot_exp[tn.slot_off + i];
    }
    if (dbg && tid == 0 && first_gather) { // diagnostic: when did the slot table arrive?
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      dbg[blockIdx.x * 8 + 5] = __builtin_amdgcn_s_memrealtime();
    }
    if (MODE != 4) {
#pragma unroll
      for (int k = 0; k < U; ++k) xr[k] = x[idx[k]];
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k) xr[k] = V(idx[k]);
    }
  };
  // the group's first tile comes from a per-group copy: its descriptor does not
  // wait for group_ptr (one dependent round trip less before the first x gather)
  const Tile tfirst = d.gfirst[g];
  if (dbg && tid == 0) dbg[blockIdx.x * 8 + 4] = __builtin_amdgcn_s_memrealtime() + (tfirst.nown & 0);
  if (t0 < t1) gather_x(tfirst);
  first_gather = false;
  if (dbg && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    dbg[blockIdx.x * 8 + 6] = __builtin_amdgcn_s_memrealtime();
  }

  for (int ti = t0; ti < t1; ++ti) {
    const Tile t = ti == t0 ? tfirst : d.tiles[ti];
    const int nown = t.nown, nslots = t.nslots;
    const unsigned ny = OFFB ? (unsigned)t.ny : (unsigned)nslots; // slots with a y window
    const int vrow0 = t.vrow_off, nvr = t.nvrows;
    const V *tv = d.vals + t.nnz_off;
    const uint16_t *ts = d.slots + t.sl_off;
    const uint4 *smeta = d.slice_meta + t.slice_base;
    const int nsl = t.nslices;
    // leader lanes of this wave's first two slices: requested before the window
    // fill waits for the x gather, so that they are there when the head packet's
    // slot address needs them (one byte per lane; padded, clamped)
    const uint8_t *llp = d.leadlane + (size_t)t.slice_base * 64 + lane;
    int L_c = llp[min(wave, max(nsl, 1) - 1) * 64];
    int L_n = llp[min(wave + NW, max(nsl, 1) - 1) * 64];

    // fill both LDS windows.  A thread owns the same slot indices here and in the
    // flush at the end of the previous tile, so no barrier is needed between.
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int i = tid + k * BLOCK;
      if (i < nslots) {
        xl[i] = xr[k];
        yl.zero(i);
        if (DET) exl[i] = er[k];
      }
    }
    if (DET) { // biased exponent field of the largest |x| this thread brought in
      int ex = 0;
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (tid + k * BLOCK < nslots) {
          const double ax = fabs((double)xr[k]);
          ex = max(ex, (int)((unsigned long long)__double_as_longlong(ax) >> 52));
        }
      // ... and of the x values its FAR entries (HYB) gather from outside the window: the
      // scale covers them too (a second pass over their columns, L2 hits later)
      for (int fp = wave; fp < ((t.nfar + 255) >> 8); fp += NW) {
        const int4 cc = *reinterpret_cast<const int4 *>(d.fcols + (size_t)t.far_off + (size_t)fp * 256u + lane * 4);
        const int e0 = fp * 256 + lane * 4;
        const int cq[4] = {cc.x, cc.y, cc.z, cc.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (e0 + u < t.nfar) {
            const double ax = fabs((double)x[cq[u]]);
            ex = max(ex, (int)((unsigned long long)__double_as_longlong(ax) >> 52));
          }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ex = max(ex, __shfl_xor(ex, o));
      if (lane == 0) atomicMax(&cfs_ticket[2 + det_parity], ex);
    }
    // the matrix stream does not depend on x: this wave's first slice header and
    // head packet (and its first COO packet) are requested BEFORE the barrier --
    // but after the window fill, so that the fill (and with it the barrier) waits
    // for the x gather only and not for these HBM loads.  Slices are handed out dynamically (they are sorted by cost, so
    // this is longest-first scheduling over the waves): a wave starts with
    // slices `wave` and `wave + NW` and draws every later one from an LDS
    // ticket counter one slice ahead of its use.
    int s = wave, s_n = wave + NW;
    uint4 meta_c = make_uint4(0u, 0u, 0u, 0u), meta_n = meta_c;
    uint32_t info_c = 0u;
    V dg_c = V(0);
    Pkt<V> N;
    N.v[0] = N.v[1] = N.v[2] = N.v[3] = V(0);
    N.c = make_ushort4(0, 0, 0, 0);
    int lr_c = 0; // rank of this lane's leader in the current slice
    if (s < nsl) {
      meta_c = smeta[s];
      if (s_n < nsl) meta_n = smeta[s_n];
      const int p0 = s * 64 + lane, q0 = min(p0, nvr - 1);
      const uint32_t i0 = stream_load<NT>(d.rowinfo + vrow0 + q0); // unconditional, clamped
      const V d0 = stream_load<NT>(d.diag + vrow0 + q0);
      info_c = p0 < nvr ? i0 : 0u;
      dg_c = p0 < nvr ? d0 : V(0);
      const unsigned long long lead0 = ((unsigned long long)meta_c.w << 32) | meta_c.z;
      lr_c = leader_rank(lead0, L_c & 63) | (L_c & 0xc0); // bits 6 / 7: sibling chain (entry_combined)
      fetch_packet<NT>(N, tv, ts, meta_c.x, meta_c.y & 0x1ffffffu, (int)(meta_c.y >> 25), lead0,
                       lane, lr_c & 63);
    }
    const int ncp = (t.ncoo + 255) >> 8; // COO packets of this tile
    Pkt<V> C;
    ushort4 Cr = make_ushort4(0, 0, 0, 0);
    C.v[0] = C.v[1] = C.v[2] = C.v[3] = V(0);
    C.c = Cr;
    if (wave < ncp) {
      fetch_packet<NT>(C, d.cvals + t.coo_off, d.ccols + t.coo_off, (uint32_t)wave * 256u,
                       (uint32_t)wave * 256u, 64, ~0ull, lane, lane);
      {
        const cfs_us4 rr = stream_load<NT>(reinterpret_cast<const cfs_us4 *>(d.crows + t.coo_off + wave * 256 + lane * 4));
        Cr = make_ushort4(rr.x, rr.y, rr.z, rr.w);
      }
    }
    if (tid == 0) cfs_ticket[0] = 2 * NW;
    __syncthreads();
    double det_unscale = 1.0;
    if (DET) {
      // |x| < 2^(E - 1022) in this window; the slots bring their own row bound (YWin)
      const int xe = __builtin_amdgcn_readfirstlane(cfs_ticket[2 + det_parity]);
      yl.xe = xe - 1022;
      // a NaN / Inf in the window of x (exponent field 2047) has no fixed-point image: every
      // row of the tile reads NaN, as the floating-point path would propagate it -- never
      // plausible finite garbage
      if (xe >= 2047) det_unscale = __longlong_as_double(0x7ff8000000000000ll);
      det_parity ^= 1;
      if (tid == 0) cfs_ticket[2 + det_parity] = 0; // the next tile's word (see the header comment)
    }
    if (dbg && tid == 0 && ti == t0) dbg[blockIdx.x * 8 + 1] = __builtin_amdgcn_s_memrealtime();

    while (MODE != 3 && s < nsl) {
      const uint32_t info = info_c;
      const V dg = dg_c;
      uint32_t off = meta_c.x, soff = meta_c.y & 0x1ffffffu;
      int cnt = (int)(meta_c.y >> 25);
      const unsigned long long leaders = ((unsigned long long)meta_c.w << 32) | meta_c.z;
      Pkt<V> A = N;
      const int lr = lr_c & 63; // leader rank of this lane in the current slice
      // COMB: one atomic per run of sibling lanes (entry_combined); a schedule with few such
      // runs -- one unknown per mesh node -- launches the plain instantiation
      const bool give = MODE == 0 && COMB && (lr_c & 64), take = MODE == 0 && COMB && (lr_c & 128);
      // ticket for the slice after next (its metadata is a scalar load that
      // lands long before it is needed)
      int s_nn = 0;
      if (lane == 0) s_nn = atomicAdd(&cfs_ticket[0], 1);
      s_nn = __builtin_amdgcn_readfirstlane(s_nn);
      const bool have_next = s_n < nsl;
      if (have_next) { // next slice: header + head packet, a whole slice ahead
        const int pn = s_n * 64 + lane, qn = min(pn, nvr - 1);
        const uint32_t in_ = stream_load<NT>(d.rowinfo + vrow0 + qn); // unconditional, clamped
        const V dn = stream_load<NT>(d.diag + vrow0 + qn);
        info_c = pn < nvr ? in_ : 0u;
        dg_c = pn < nvr ? dn : V(0);
        const unsigned long long lead_n = ((unsigned long long)meta_n.w << 32) | meta_n.z;
        lr_c = leader_rank(lead_n, L_n & 63) | (L_n & 0xc0); // L_n was requested a slice ago
        fetch_packet<NT>(N, tv, ts, meta_n.x, meta_n.y & 0x1ffffffu, (int)(meta_n.y >> 25), lead_n,
                         lane, lr_c & 63);
      }
      meta_c = meta_n;
      if (s_nn < nsl) meta_n = smeta[s_nn];
      L_n = llp[min(s_nn, nsl - 1) * 64]; // leader lanes of the slice after next
      const int s_cur = s;
      s = s_n;
      s_n = s_nn;

      const int r = info & 0xffffu;
      const int a = (int)(info >> 16); // packets of this lane's row
      const V xi = xl[r];
      V acc = V(0);
      const int amax = __builtin_amdgcn_readfirstlane(a); // rows are sorted: lane 0 is longest

      int g = 0;
      Pkt<V> B;
      auto consume = [&](const Pkt<V> &pk, bool act) {
        if (MODE == 0 && COMB) consume_combined<V, OFFB, DET>(pk, xl, yl, xi, acc, ny, act, give, take);
        else if (act) consume_packet<V, MODE, OFFB, DET>(pk, xl, yl, xi, acc, ny);
      };
      while (g + 2 < amax) { // steady state: two packets per trip, no copies
        const int cnt1 = __popcll(__ballot(a > g + 1));
        const uint32_t off1 = off + 4u * (uint32_t)cnt, soff1 = soff + slot_block(leaders, cnt);
        fetch_packet<NT>(B, tv, ts, off1, soff1, cnt1, leaders, lane, lr);
        consume(A, a > g);
        const int cnt2 = __popcll(__ballot(a > g + 2));
        const uint32_t off2 = off1 + 4u * (uint32_t)cnt1, soff2 = soff1 + slot_block(leaders, cnt1);
        fetch_packet<NT>(A, tv, ts, off2, soff2, cnt2, leaders, lane, lr);
        consume(B, a > g + 1);
        g += 2;
        off = off2;
        soff = soff2;
        cnt = cnt2;
      }
      if (amax - g == 2) {
        const int cnt1 = __popcll(__ballot(a > g + 1));
        fetch_packet<NT>(B, tv, ts, off + 4u * (uint32_t)cnt, soff + slot_block(leaders, cnt), cnt1,
                         leaders, lane, lr);
        consume(A, a > g);
        consume(B, a > g + 1);
      } else if (amax - g == 1) {
        consume(A, a > g);
      }
      if (s_cur * 64 + lane < nvr) yl.add(r, (double)fma(dg, xi, acc));
    }
    // COO leftovers: packet p = wave, wave + NW, ...; the first one was requested
    // at the top of the tile
    for (int cp = wave; MODE != 3 && cp < ncp; cp += NW) {
      const Pkt<V> Q = C;
      const ushort4 Qr = Cr;
      if (cp + NW < ncp) {
        fetch_packet<NT>(C, d.cvals + t.coo_off, d.ccols + t.coo_off, (uint32_t)(cp + NW) * 256u,
                         (uint32_t)(cp + NW) * 256u, 64, ~0ull, lane, lane);
        const cfs_us4 rr = stream_load<NT>(reinterpret_cast<const cfs_us4 *>(d.crows + t.coo_off + (cp + NW) * 256 + lane * 4));
        Cr = make_ushort4(rr.x, rr.y, rr.z, rr.w);
      }
      const int e0 = cp * 256 + lane * 4;
      if (e0 + 0 < t.ncoo) coo_update<V, MODE, OFFB, DET>(xl, yl, Q.v[0], Qr.x, Q.c.x, ny);
      if (e0 + 1 < t.ncoo) coo_update<V, MODE, OFFB, DET>(xl, yl, Q.v[1], Qr.y, Q.c.y, ny);
      if (e0 + 2 < t.ncoo) coo_update<V, MODE, OFFB, DET>(xl, yl, Q.v[2], Qr.z, Q.c.z, ny);
      if (e0 + 3 < t.ncoo) coo_update<V, MODE, OFFB, DET>(xl, yl, Q.v[3], Qr.w, Q.c.w, ny);
    }
    // FAR entries (HYB): a = A[row(r)][col] with col outside this tile and used only
    // once by it -- or the mirror image of such an entry of another tile.  One-sided:
    // y_l[r] += a * x[col], x gathered from global memory (L2): no slot, no strip
    for (int fp = wave; MODE != 3 && fp < ((t.nfar + 255) >> 8); fp += NW) {
      const size_t base = (size_t)t.far_off + (size_t)fp * 256u;
      V fv[4];
      if (sizeof(V) == 8) {
        const cfs_d2 lo = *reinterpret_cast<const cfs_d2 *>(d.fvals + base + lane * 2);
        const cfs_d2 hi = *reinterpret_cast<const cfs_d2 *>(d.fvals + base + 128 + lane * 2);
        fv[0] = lo.x; fv[1] = lo.y; fv[2] = hi.x; fv[3] = hi.y;
      } else {
        const cfs_f4 q4 = *reinterpret_cast<const cfs_f4 *>(d.fvals + base + lane * 4);
        fv[0] = q4.x; fv[1] = q4.y; fv[2] = q4.z; fv[3] = q4.w;
      }
      const cfs_us4 rr = *reinterpret_cast<const cfs_us4 *>(d.frows + base + lane * 4);
      const int4 cc = *reinterpret_cast<const int4 *>(d.fcols + base + lane * 4);
      const V x0 = x[cc.x], x1 = x[cc.y], x2 = x[cc.z], x3 = x[cc.w]; // padding: column 0
      const int e0 = fp * 256 + lane * 4;
      // (deterministic build: the tile's scale covers these x values too, see the window fill)
      if (e0 + 0 < t.nfar) yl.add(rr.x, (double)fv[0] * (double)x0);
      if (e0 + 1 < t.nfar) yl.add(rr.y, (double)fv[1] * (double)x1);
      if (e0 + 2 < t.nfar) yl.add(rr.z, (double)fv[2] * (double)x2);
      if (e0 + 3 < t.nfar) yl.add(rr.w, (double)fv[3] * (double)x3);
    }
    if (dbg && lane == 0 && wave == 0 && ti + 1 == t1) dbg[blockIdx.x * 8 + 7] = __builtin_amdgcn_s_memrealtime();
    if (ti + 1 < t1) gather_x(d.tiles[ti + 1]); // lands behind the barrier + flush
    // y positions of the own rows (original numbering, block-local): requested
    // before the barrier, used by the flush after it
    int yidx[U];
#pragma unroll
    for (int k = 0; k < U; ++k)
      yidx[k] = d.slot_col[t.slot_off + min(tid + k * BLOCK, nown - 1)] - d.row_begin;
    __syncthreads();
    if (dbg && tid == 0 && ti + 1 == t1) dbg[blockIdx.x * 8 + 2] = __builtin_amdgcn_s_memrealtime();
    // flush the y window: own rows -> y, halo sums -> this tile's strip.  Plain
    // stores; y is fully overwritten.
    if (MODE != 4) {
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int i = tid + k * BLOCK;
        if (i < nown) y[yidx[k]] = (V)yl.get(i, det_unscale);
        else if (i < (int)ny) d.strip[t.halo_off + (i - nown)] = (V)yl.get(i, det_unscale);
      }
    }
  }
  if (dbg && tid == 0) dbg[blockIdx.x * 8 + 3] = __builtin_amdgcn_s_memrealtime();
}

// halo fold: y[dst] += sum of the strip entries aimed at dst, in a fixed order.
// One 16-byte record per destination {dst, e0, e1, e2}: up to three strip entries
// are inlined (e1 / e2 = -1 when absent), so the common destination costs two
// dependent round trips: the record, then y[dst] and its entries all in flight
// together.  A longer list keeps e0, e1 in the record and e2 = -(offset + 2) of
// its remainder in `fidx`: [count, entry 2, entry 3, ...].  A lane sums the next
// 16 entries itself, four loads in flight at a time; what is left of a very long
// list (a hub row collects contributions from many tiles) is summed by the whole
// wave, strided, with a fixed shuffle tree -- one slow lane would otherwise
// decide the duration of the launch.  The order of the additions is fixed.
template <typename V>
__global__ void __launch_bounds__(256)
    cfs_fold_kernel(V *__restrict__ y, const V *__restrict__ src,
                    const int4 *__restrict__ frec, const int32_t *__restrict__ fidx, int m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int r = 0, b = 0, e = 0;
  V s = V(0);
  if (i < m) {
    const int4 rec = frec[i];
    r = rec.x;
    const V y0 = y[r];
    const V s0 = src[rec.y];
    const V s1 = src[max(rec.z, 0)]; // unconditional, clamped: all in flight together
    const V s2 = src[max(rec.w, 0)];
    s = y0 + s0;
    if (rec.z >= 0) s += s1;
    if (rec.w >= 0) s += s2;
    if (rec.w < -1) {
      b = -(rec.w + 2);
      e = b + 1 + fidx[b];
      b += 1;
    }
  }
  const int own_end = min(e, b + 16);
  for (int q = b; q < own_end; q += 4) {
    int j[4];
    V v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) j[u] = fidx[min(q + u, own_end - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[j[u]];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (q + u < own_end) s += v[u];
  }
  unsigned long long need = __ballot(e > own_end);
  while (need) {
    const int L = __ffsll((long long)need) - 1;
    need &= need - 1;
    const int lb = __shfl(own_end, L), le = __shfl(e, L);
    V p = V(0);
    for (int q = lb + lane; q < le; q += 64) p += src[fidx[q]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p += __shfl_down(p, o);
    const V tot = __shfl(p, 0);
    if (lane == L) s += tot;
  }
  if (i < m) y[r] = s;
}

// new values into an existing schedule (cfs_hip_sym_update_values_*): every entry of a
// value array of the device format takes the caller's value at its recorded position
// (GPU-side packing of the values: the sparsity pattern, and with it the whole schedule
// -- tiles, slots, leaders, fold index -- stays)
template <typename V>
__global__ void __launch_bounds__(256)
    cfs_value_scatter_kernel(V *__restrict__ dst, const int32_t *__restrict__ map,
                             const V *__restrict__ src, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int32_t m = map[i];
    dst[i] = m >= 0 ? src[m] : V(0);
  }
}

// the diagonal of the rows a handle owns, out of its schedule (cfs_hip_sym_diagonal_async): a
// workgroup per tile.  `diag` is per VIRTUAL row, in the tile's sorted order, and holds a_ii on the
// first chunk of a row only -- the other chunks of a split row, and a row without a stored diagonal
// entry, hold +0 -- so at most one virtual row of a local row carries a non-zero word: it is put
// into the row's place of an LDS window of the tile's own rows (zeroed first: no two lanes write one
// word, no atomics), and the window leaves through the own-row slots of slot_col, which name the
// caller's row of every local row (consecutive in natural order: coalesced stores; a permutation
// inside the tile's cluster otherwise).  Every owned row lies in exactly one tile (cfs_hip_sym_
// plan_check_*), so every entry of `out` is written exactly once and nothing has to be zeroed first.
template <typename V>
__global__ void __launch_bounds__(256)
    cfs_diag_gather_kernel(V *__restrict__ out, const Tile *__restrict__ tiles, int ntiles,
                           const int32_t *__restrict__ slot_col, const uint32_t *__restrict__ rowinfo,
                           const V *__restrict__ diag, int row_begin, int rows, int window) {
  extern __shared__ __align__(16) unsigned char cfs_diag_smem[];
  V *w = reinterpret_cast<V *>(cfs_diag_smem);
  typedef typename std::conditional<sizeof(V) == 8, unsigned long long, unsigned>::type Bits;
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const int nown = min(tiles[ti].nown, window), nvr = tiles[ti].nvrows, v0 = tiles[ti].vrow_off,
              s0 = tiles[ti].slot_off;
    for (int i = threadIdx.x; i < nown; i += 256) w[i] = V(0);
    __syncthreads();
    for (int v = threadIdx.x; v < nvr; v += 256) {
      const V d = diag[v0 + v];
      const int r = (int)(rowinfo[v0 + v] & 0xffffu);
      Bits bits;
      __builtin_memcpy(&bits, &d, sizeof bits);
      if (bits != 0 && r < nown) w[r] = d; // (the bits, not the value: a stored -0 or NaN is copied too)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nown; i += 256) {
      const int o = slot_col[s0 + i] - row_begin;
      if ((unsigned)o < (unsigned)rows) out[o] = w[i];
    }
    __syncthreads(); // the next tile zeroes the window
  }
}

// the bs x bs diagonal blocks of a whole matrix, out of its schedule (cfs_hip_sym_block_diagonal_async):
// out[k bs^2 + (i mod bs) bs + (j mod bs)] = a_ij for i, j in block k, both triangles.  `out` is zeroed
// in front of the launch.  A workgroup per tile, as above.  The diagonal positions take the words of
// `diag` through the same LDS window as cfs_diag_gather_kernel, so they are its bits.  The off-diagonal
// positions are found by walking the tile's stored entries the way cfs_plan::decode_plan does on the
// host: a wave per slice (rowinfo packet counts, lanes per packet by ballot, the leader's rank for the
// slot block), then the COO section up to ncoo and the far section up to nfar_low -- the mirror images
// [nfar_low, nfar) repeat entries another tile has already delivered.  Row and column of an entry come
// back to the caller's numbering through slot_col (far columns are stored in it already); in clustered
// order the stored orientation follows the schedule, hence (hi, lo) = (max, min).  An entry inside a
// block is added to both of its positions: atomics, because a matrix may store a position twice (the
// SpMV sums them too) and because the two triangles of a block may come from different tiles.  Set-up
// work, one pass over the index stream; every lane reads single words.
template <typename V>
__global__ void __launch_bounds__(256)
    cfs_block_gather_kernel(V *__restrict__ out, const Tile *__restrict__ tiles, int ntiles, SymDev<V> d, int n, int bs,
                            int window) {
  extern __shared__ __align__(16) unsigned char cfs_block_smem[];
  V *w = reinterpret_cast<V *>(cfs_block_smem);
  typedef typename std::conditional<sizeof(V) == 8, unsigned long long, unsigned>::type Bits;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto val_pos = [](int l, int j, int cnt) { // cfs_plan::packet_val_pos
    return sizeof(V) == 8 ? (j >> 1) * 2 * cnt + l * 2 + (j & 1) : l * 4 + j;
  };
  auto put = [&](int a, int b, V v) {
    const int hi = max(a, b), lo = min(a, b);
    if (hi == lo || lo < 0 || hi >= n || hi / bs != lo / bs) return;
    V *blk = out + (size_t)(hi / bs) * (size_t)(bs * bs);
    const int i = hi % bs, j = lo % bs;
    atomicAdd(blk + i * bs + j, v);
    atomicAdd(blk + j * bs + i, v);
  };
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const Tile t = tiles[ti];
    const int nown = min(t.nown, window), nvr = t.nvrows;
    const int32_t *sc = d.slot_col + t.slot_off;
    // the diagonal, as cfs_diag_gather_kernel
    for (int i = threadIdx.x; i < nown; i += 256) w[i] = V(0);
    __syncthreads();
    for (int v = threadIdx.x; v < nvr; v += 256) {
      const V dg = d.diag[t.vrow_off + v];
      const int r = (int)(d.rowinfo[t.vrow_off + v] & 0xffffu);
      Bits bits;
      __builtin_memcpy(&bits, &dg, sizeof bits);
      if (bits != 0 && r < nown) w[r] = dg; // (a split row's other chunks hold +0 and do not overwrite)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nown; i += 256) {
      const int o = sc[i];
      if ((unsigned)o < (unsigned)n) out[(size_t)(o / bs) * (size_t)(bs * bs) + (size_t)(o % bs) * (bs + 1)] = w[i];
    }
    // packets: wave `wave` walks slices wave, wave + 4, ...
    const V *tv = d.vals + t.nnz_off;
    const uint16_t *ts = d.slots + t.sl_off;
    for (int s = wave; s < t.nslices; s += 4) {
      const int p0 = s * 64 + lane;
      const uint32_t info = p0 < nvr ? d.rowinfo[t.vrow_off + p0] : 0u;
      const int r = (int)(info & 0xffffu), a = (int)(info >> 16);
      const uint4 sm = d.slice_meta[t.slice_base + s];
      const unsigned long long leaders = ((unsigned long long)sm.w << 32) | sm.z;
      long long o = sm.x, os = sm.y & 0x1ffffffu;
      const int Ld = d.leadlane[(size_t)(t.slice_base + s) * 64 + lane] & 63;
      const int rank = leader_rank(leaders, Ld);
      const int row = p0 < nvr ? sc[r] : -1;
      const int amax = __builtin_amdgcn_readfirstlane(a); // rows are sorted: lane 0 is longest
      for (int g = 0; g < amax; ++g) {
        const int cnt = __popcll(__ballot(a > g));
        if (a > g) {
#pragma unroll
          for (int j = 0; j < 4; ++j) put(row, sc[ts[os + rank * 4 + j]], tv[o + val_pos(lane, j, cnt)]);
        }
        o += 4 * (long long)cnt;
        os += 4 * (long long)active_leaders(leaders, cnt);
      }
    }
    // COO leftovers and the lower far entries: 256-entry packets, slots at [lane][4]
    for (int e = threadIdx.x; e < t.ncoo; e += 256) {
      const size_t pk = (size_t)t.coo_off + (size_t)(e & ~255);
      put(sc[d.crows[(size_t)t.coo_off + e]], sc[d.ccols[(size_t)t.coo_off + e]],
          d.cvals[pk + val_pos((e & 255) >> 2, e & 3, 64)]);
    }
    for (int e = threadIdx.x; e < t.nfar_low; e += 256) {
      const size_t pk = (size_t)t.far_off + (size_t)(e & ~255);
      put(sc[d.frows[(size_t)t.far_off + e]], d.fcols[(size_t)t.far_off + e],
          d.fvals[pk + val_pos((e & 255) >> 2, e & 3, 64)]);
    }
    __syncthreads(); // the next tile zeroes the window
  }
}

// pack contributions for rows owned by lower ranks: one value per remote row
template <typename V>
__global__ void __launch_bounds__(256)
    cfs_pack_kernel(V *__restrict__ send, const V *__restrict__ src,
                    const int32_t *__restrict__ sptr, const int32_t *__restrict__ sidx,
                    int m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  V s = V(0);
  for (int q = sptr[i]; q < sptr[i + 1]; ++q) s += src[sidx[q]];
  send[i] = s;
}

// ---------------------------------------------------------------------------
// host objects
// ---------------------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel FUNCTION (one
// template instantiation, per device), not to a handle: two handles with different
// windows share instantiations.  Every instantiation is raised ONCE per device to
// the ceiling of a CU (160 KiB minus the static ticket counter) and never lowered.
static int raise_lds_limit(const void *kernel, int device) {
  static std::mutex mu;
  static std::vector<std::pair<const void *, int>> done;
  std::lock_guard<std::mutex> lk(mu);
  for (auto &d : done)
    if (d.first == kernel && d.second == device) return 0;
  HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             160 * 1024 - 64));
  done.push_back({kernel, device});
  return 0;
}

// fold records {dst, e0, e1, e2 | -(offset + 2)} and the remainder lists
// [count, entries 2..] of destinations with more than three contributions
// (see cfs_fold_kernel)
static void make_fold_records(const std::vector<int32_t> &dst, const std::vector<int32_t> &ptr,
                              const std::vector<int32_t> &idx, std::vector<int4> &rec,
                              std::vector<int32_t> &rest) {
  cfs_planfile::make_fold_records(dst, ptr, idx, rec, rest, [](int a, int b, int c, int d) { return make_int4(a, b, c, d); });
}
static_assert(sizeof(int4) == sizeof(cfs_planfile::FoldRec), "a plan file stores fold records as int4");

// staging of a handle for callers that pass HOST pointers (the reference's API
// hands raw host pointers every call, include/kernel/sparse_kernel.hpp:22-23):
// device mirrors of x / y, and page-locked blocks from the pinned pool
// (CFS_HIP_MEM_PINNED, allocated once per handle) that pageable vectors are
// copied through with all host threads.  A vector that already lives in
// page-locked memory (internal_alloc(.., Platform::cpu) of this build hands such
// blocks out) is DMA-ed in place.
struct HostStage {
  DevBuf xdev, ydev;
  PinBuf xpin, ypin;
};

// y <- launch(x) for x / y that may be host or device pointers, on `device`'s
// library stream.  Returns after the result is complete when host memory is
// involved; with both vectors resident the work is only enqueued.
template <class Launch>
static int run_staged(int device, HostStage &S, size_t xbytes, size_t ybytes, void *y,
                      const void *x, Launch launch) {
  cfs_rt::DevCtx *ctx;
  int rc = cfs_rt::device_ctx(device, &ctx);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  DeviceGuard g(device);
  const cfs_rt::PtrInfo xi = cfs_rt::classify(x), yi = cfs_rt::classify(y);
  if ((xi.device && xi.dev != device) || (yi.device && yi.dev != device))
    return set_err(CFS_HIP_ERR_ARG, "x / y live on device " +
                                        std::to_string(xi.device && xi.dev != device ? xi.dev : yi.dev) +
                                        ", the matrix on device " + std::to_string(device));
  const void *xdev = x;
  void *ydev = y;
  if (!xi.device) {
    if (S.xdev.bytes < xbytes && (rc = S.xdev.alloc(xbytes))) return rc;
    const void *src = x;
    if (!xi.pinned) { // pageable: through the handle's page-locked block
      if ((rc = S.xpin.reserve(xbytes))) return rc;
      cfs_rt::parallel_copy(S.xpin.p, x, xbytes);
      src = S.xpin.p;
    }
    HIPCHK(hipMemcpyAsync(S.xdev.p, src, xbytes, hipMemcpyHostToDevice, st));
    xdev = S.xdev.p;
  }
  if (!yi.device) {
    if (S.ydev.bytes < ybytes && (rc = S.ydev.alloc(ybytes))) return rc;
    ydev = S.ydev.p;
  }
  if ((rc = launch(ydev, xdev, st))) return rc;
  if (!yi.device) {
    if (yi.pinned) {
      HIPCHK(hipMemcpyAsync(y, ydev, ybytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    } else {
      if ((rc = S.ypin.reserve(ybytes))) return rc;
      HIPCHK(hipMemcpyAsync(S.ypin.p, ydev, ybytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      cfs_rt::parallel_copy(y, S.ypin.p, ybytes);
    }
  } else if (!xi.device) {
    HIPCHK(hipStreamSynchronize(st)); // the staged x may be overwritten by the next call
  }
  // both resident: enqueued on the library stream (a BLOCKING stream: a caller's
  // own hipMemcpy / hipDeviceSynchronize on the null stream orders behind it, and
  // so do cfs_hip_memcpy / cfs_hip_synchronize)
  return 0;
}

struct cfs_hip_sym_s {
  int value_bytes = 8;
  virtual ~cfs_hip_sym_s() {}
  virtual int spmv_local(void *y, const void *x, void *send, hipStream_t st, int phases = 7) = 0;
  virtual int recv_fold(void *y, const void *recv, hipStream_t st) = 0;
  virtual int set_recv(int nrecv, const int *rows) = 0;
  virtual void stats(cfs_hip_sym_stats *o) = 0;
  virtual const std::vector<int32_t> &send_counts() = 0;
  virtual const std::vector<int32_t> &send_rows() = 0;
  virtual int n() = 0;
  virtual int rows() = 0;
  virtual int timeline(void *y, const void *x, unsigned long long *host, int cap, int *ngroups) = 0;
  virtual int group_features(long long *out, int cap, int *ngroups) = 0;
  // values_dev: the caller's full CSR value array (same pattern as at create), on this device
  virtual int update_values(const void *values_dev, long long nnz, hipStream_t st) = 0;
  // d_dev[i - row_begin] = a_ii of the owned rows, from the device arrays (cfs_hip_sym_diagonal_async)
  virtual int diagonal(void *d_dev, hipStream_t st) = 0;
  // the block_rows x block_rows diagonal blocks of a whole matrix on one device, zeroing included
  // (cfs_hip_sym_block_diagonal_async); a shard or a multi-device handle has no such thing: a block
  // straddles the row splits
  virtual int block_diagonal(void *, int, hipStream_t) {
    return cfs_rt::set_err(CFS_HIP_ERR_UNSUPPORTED, "block diagonal: a handle of the whole matrix on one device (blocks "
                                                    "straddle the row splits of a multi-device handle)");
  }
  int device = 0; // the device this handle's arrays live on (current device at create)
  unsigned long long values_epoch = 0; // cfs_hip_sym_update_values_* so far: a refreshable hierarchy sees that level 0 changed
  std::string plan_note; // why the device builder handed the schedule to the host builder ("" = it did not)
  HostStage stage; // host-pointer callers
  // the last (y, x) pair whose placement was validated (async entry points)
  const void *ok_x = nullptr, *ok_y = nullptr;
};

template <typename V> struct SymMatrix : cfs_hip_sym_s {
  SymPlan<V> P; // big arrays released after upload
  DevBuf tiles, gfirst, group_ptr, slot_col, rowinfo, diag, slice_meta, leadlane, vals, slots, strip;
  DevBuf cvals, crows, ccols, fvals, frows, fcols;
  DevBuf val_map, cval_map, fval_map, diag_map; // CFS_HIP_FLAG_KEEP_VALUE_MAP
  bool has_value_map = false;
  int64_t nnz_caller = 0; // entries of the caller's CSR the maps point into
  DevBuf fold_rec, fold_idx, send_ptr, send_idx;
  DevBuf slot_exp; // deterministic build: scale exponent of every slot
  const short *dev_slot_exp = nullptr;
  DevBuf rfold_rec, rfold_idx;
  SymDev<V> dev{};
  int nfold = 0, nsend = 0, nrfold = 0;
  int ablate_mode = 0; // cfs_hip_options.flags & 7 (timing-only ablations)
  bool nt_stream = true; // matrix stream larger than the Infinity Cache: non-temporal loads
  bool offblock = false; // some tile has one-sided (off-block) slots: mirrored shard
  bool combine_ok = false; // enough sibling chains (>= 10 % of the lane-packets) for the combining kernel
  bool combine = false;    // ... and it is the one this handle launches
  bool combine_forced = false;
  int64_t mirror_entries = 0;
  unsigned long long *dbg_buf = nullptr; // set only by cfs_hip_sym_debug_timeline
  size_t lds_bytes = 0;
  int64_t halo_slots = 0, stream_len = 0, slot_len = 0, nslices = 0, coo_len = 0, far_len = 0, far_entries = 0;

  bool device_built = false; // the schedule was built by cfs_devplan.hpp (arrays never on the host)
  int build_flags = 0, num_cus = 0; // what a plan file records: the caller's option flags, the CUs the grid was sized for

  // the size rules of the two kernel choices (finish_setup; tune() may overrule the first by measurement)
  static bool size_rule_combine(const SymPlan<V> &P) {
    return P.chained_packets * 10 >= P.lane_packets && P.chained_packets > 0 &&
           P.stream_len * (int64_t)sizeof(V) + P.slot_len * 2 >= (int64_t)200 * 1000 * 1000;
  }
  static bool size_rule_nt(const SymPlan<V> &P) {
    return (P.stream_len * (int64_t)sizeof(V) + P.slot_len * 2) > (int64_t)240 * 1024 * 1024;
  }

  int upload() {
    int rc;
#define UP(buf, vec)                                                          \
  if ((rc = buf.upload(vec.data(), vec.size() * sizeof(vec[0])))) return rc;
    UP(tiles, P.tiles)
    UP(slot_col, P.slot_col)
    UP(rowinfo, P.rowinfo)
    UP(diag, P.diag)
    UP(slice_meta, P.slice_meta)
    UP(leadlane, P.leadlane)
    UP(cvals, P.cvals)
    UP(crows, P.crows)
    UP(ccols, P.ccols)
    UP(vals, P.vals)
    UP(slots, P.slots)
    UP(fvals, P.fvals)
    UP(frows, P.frows)
    UP(fcols, P.fcols)
    has_value_map = !P.val_map.empty();
    if (has_value_map) {
      UP(val_map, P.val_map)
      UP(cval_map, P.cval_map)
      UP(fval_map, P.fval_map)
      UP(diag_map, P.diag_map)
      cfs_plan::release_async(P.val_map);
      std::vector<int32_t>().swap(P.cval_map);
      std::vector<int32_t>().swap(P.fval_map);
      std::vector<int32_t>().swap(P.diag_map);
    }
    {
      std::vector<int4> rec;
      std::vector<int32_t> rest;
      make_fold_records(P.fold_dst, P.fold_ptr, P.fold_idx, rec, rest);
      if ((rc = fold_rec.upload(rec.data(), rec.size() * sizeof(int4)))) return rc;
      if ((rc = fold_idx.upload(rest.data(), rest.size() * 4))) return rc;
    }
    UP(send_ptr, P.send_ptr)
    UP(send_idx, P.send_idx)
    if (P.deterministic) {
      UP(slot_exp, P.slot_exp)
      dev_slot_exp = (const short *)slot_exp.p;
    }
#undef UP
    if ((rc = finish_setup((int64_t)P.slice_meta.size()))) return rc;
    // release the big host arrays; keep the small metadata
    cfs_plan::release_async(P.vals);
    cfs_plan::release(P.slots);
    std::vector<uint8_t>().swap(P.leadlane);
    std::vector<V>().swap(P.cvals);
    std::vector<uint16_t>().swap(P.crows);
    std::vector<uint16_t>().swap(P.ccols);
    std::vector<V>().swap(P.fvals);
    std::vector<uint16_t>().swap(P.frows);
    std::vector<int32_t>().swap(P.fcols);
    std::vector<V>().swap(P.diag);
    std::vector<uint32_t>().swap(P.rowinfo);
    std::vector<int32_t>().swap(P.fold_idx);
    std::vector<int32_t>().swap(P.send_idx);
    return 0;
  }
  // the schedule's arrays were built in place by the device builder: only the launch
  // tables and the derived settings are left to do
  int adopt_device_schedule() {
    device_built = true;
    int64_t ns = 0;
    for (const Tile &t : P.tiles) ns += t.nslices;
    return finish_setup(ns);
  }

  // what both builders share once the arrays are on the device: launch-slot tables, strips,
  // kernel choice, LDS window, staging room, cache policy
  int finish_setup(int64_t nslices_in) {
    int rc;
    { // per launch slot: first tile + tile range of the group that runs there
      const int G = (int)P.group_first.size();
      std::vector<Tile> gf(G);
      std::vector<int2> gr(G);
      for (int sl = 0; sl < G; sl++) {
        const int g = (int)P.launch_order.size() == G ? P.launch_order[sl] : sl;
        gf[sl] = P.group_first[g];
        gr[sl] = make_int2(P.group_ptr[g], P.group_ptr[g + 1]);
      }
      if ((rc = gfirst.upload(gf.data(), gf.size() * sizeof(Tile)))) return rc;
      if ((rc = group_ptr.upload(gr.data(), gr.size() * sizeof(int2)))) return rc;
    }
    if ((rc = strip.alloc((size_t)P.nhalo * sizeof(V)))) return rc;
    halo_slots = P.nhalo;
    offblock = P.onesided_slots > 0;
    // combining kernel: enough sibling chains, and a launch long enough for the longer
    // dependency chain per entry to hide (measured: ldoor stand-in, 283 MB per launch,
    // +3 %; 1/8 shards, 89-131 MB, -8 %); tune() times both where it may (sym_create)
    combine_ok = P.chained_packets * 10 >= P.lane_packets && P.chained_packets > 0;
    combine = size_rule_combine(P);
    combine_forced = false;
    // developer knob CFS_HIP_COMBINE (read only when set; a forced choice skips choose_kernel):
    // 0 = no sibling chains in the plan (to_opts), 2 = the combining kernel whatever the size
    // (when the plan has enough chains), 3 = the chained plan but the plain kernel
    if (const char *e = getenv("CFS_HIP_COMBINE")) {
      if (atoi(e) == 2) combine = combine_ok, combine_forced = true;
      if (atoi(e) == 3) combine = false, combine_forced = true;
    }
    mirror_entries = P.mirror_entries;
    stream_len = P.stream_len;
    slot_len = P.slot_len;
    nslices = nslices_in;
    coo_len = P.coo_len;
    far_len = P.far_len;
    far_entries = P.far_entries;
    nfold = (int)P.fold_dst.size();
    nsend = (int)P.send_row.size();
    dev.tiles = (const Tile *)tiles.p;
    dev.gfirst = (const Tile *)gfirst.p;
    dev.group_range = (const int2 *)group_ptr.p;
    dev.slot_col = (const int32_t *)slot_col.p;
    dev.rowinfo = (const uint32_t *)rowinfo.p;
    dev.diag = (const V *)diag.p;
    dev.slice_meta = (const uint4 *)slice_meta.p;
    dev.leadlane = (const uint8_t *)leadlane.p;
    dev.cvals = (const V *)cvals.p;
    dev.crows = (const uint16_t *)crows.p;
    dev.ccols = (const uint16_t *)ccols.p;
    dev.vals = (const V *)vals.p;
    dev.slots = (const uint16_t *)slots.p;
    dev.fvals = (const V *)fvals.p;
    dev.frows = (const uint16_t *)frows.p;
    dev.fcols = (const int32_t *)fcols.p;
    dev.strip = (V *)strip.p;
    dev.row_begin = P.row_begin;
    dev.lds_slots = P.lds_slots;
    lds_bytes = (size_t)P.lds_slots * (size_t)cfs_plan::slot_lds_bytes<V>(P.deterministic);
    // the stream is cacheable across SpMVs only if it fits the 256 MiB Infinity Cache
    nt_stream = size_rule_nt(P);
    // developer knob CFS_HIP_NT=0|1 (read only when set): cacheable / non-temporal stream
    // loads whatever the size, so that tests reach both instantiations at small sizes
    if (const char *e = getenv("CFS_HIP_NT")) nt_stream = atoi(e) != 0;
    if (getenv("CFS_PLAN_VERBOSE"))
      fprintf(stderr, "[cfs_hip] handle: %s-built, %d tiles, window %d slots, %d threads x %d per CU, sibling chains %lld of %lld "
              "lane-packets -> %s kernel, %s stream loads\n", device_built ? "device" : "host", (int)P.tiles.size(),
              P.lds_slots, P.block_threads, P.wg_per_cu, (long long)P.chained_packets, (long long)P.lane_packets,
              combine ? "combining" : "plain", nt_stream ? "non-temporal" : "cacheable");
    return 0;
  }

  // the template arguments of the tile-kernel instantiation this handle launches
  // (cfs_sym_tile_kernel<V, BLOCK, MODE, NT, OFFB, U, DET, COMB>): tile_kernel() launches
  // what this says and cfs_hip_sym_debug_kernel reports it
  struct TileVariant {
    int block, mode;
    bool nt, offb;
    int u; // 3, 6 or kSlotsPerThread: the smallest bucket that covers the window
    bool det, comb;
  };
  TileVariant tile_variant() const {
    constexpr int UM = cfs_plan::kSlotsPerThread;
    TileVariant t;
    t.block = P.block_threads == 256 ? 256 : (P.block_threads == 512 ? 512 : 1024);
    t.det = t.block != 256 && P.deterministic; // (to_opts: deterministic = 512 or 1 024 threads)
    t.mode = !t.det && ablate_mode >= 1 && ablate_mode <= 4 ? ablate_mode : 0;
    if (t.mode != 0) { // timing-only ablations: one instantiation each
      t.nt = true, t.offb = false, t.u = UM, t.comb = true;
      return t;
    }
    const int u = (P.lds_slots + P.block_threads - 1) / P.block_threads;
    t.nt = nt_stream;
    t.offb = offblock;
    t.u = u <= 3 ? 3 : (u <= 6 ? 6 : UM);
    t.comb = t.det || combine; // the deterministic instantiations always combine siblings
    return t;
  }
  template <int BLOCK> static const void *pick_kernel(const TileVariant &t) {
#define CFS_K(M, N, O, UU) ((const void *)cfs_sym_tile_kernel<V, BLOCK, M, N, O, UU>)
#define CFS_KP(N, O, UU) ((const void *)cfs_sym_tile_kernel<V, BLOCK, 0, N, O, UU, false, false>)
#define CFS_KDET(N, O, UU) ((const void *)cfs_sym_tile_kernel<V, (BLOCK < 512 ? 512 : BLOCK), 0, N, O, UU, true>)
    constexpr int UM = cfs_plan::kSlotsPerThread;
    switch (t.mode) {
    case 1: return CFS_K(1, true, false, UM);
    case 2: return CFS_K(2, true, false, UM);
    case 3: return CFS_K(3, true, false, UM);
    case 4: return CFS_K(4, true, false, UM);
    default: break;
    }
    const int ui = t.u == 3 ? 0 : (t.u == 6 ? 1 : 2);
    if (t.det) { // CFS_HIP_FLAG_DETERMINISTIC: 512 or 1 024 threads (to_opts)
      static const void *const dtab[2][2][3] = {
          {{CFS_KDET(false, false, 3), CFS_KDET(false, false, 6), CFS_KDET(false, false, UM)},
           {CFS_KDET(false, true, 3), CFS_KDET(false, true, 6), CFS_KDET(false, true, UM)}},
          {{CFS_KDET(true, false, 3), CFS_KDET(true, false, 6), CFS_KDET(true, false, UM)},
           {CFS_KDET(true, true, 3), CFS_KDET(true, true, 6), CFS_KDET(true, true, UM)}}};
      return dtab[t.nt ? 1 : 0][t.offb ? 1 : 0][ui];
    }
    static const void *const tab[2][2][3] = {
        {{CFS_K(0, false, false, 3), CFS_K(0, false, false, 6), CFS_K(0, false, false, UM)},
         {CFS_K(0, false, true, 3), CFS_K(0, false, true, 6), CFS_K(0, false, true, UM)}},
        {{CFS_K(0, true, false, 3), CFS_K(0, true, false, 6), CFS_K(0, true, false, UM)},
         {CFS_K(0, true, true, 3), CFS_K(0, true, true, 6), CFS_K(0, true, true, UM)}}};
    static const void *const ptab[2][2][3] = { // plain: no sibling-combined atomics
        {{CFS_KP(false, false, 3), CFS_KP(false, false, 6), CFS_KP(false, false, UM)},
         {CFS_KP(false, true, 3), CFS_KP(false, true, 6), CFS_KP(false, true, UM)}},
        {{CFS_KP(true, false, 3), CFS_KP(true, false, 6), CFS_KP(true, false, UM)},
         {CFS_KP(true, true, 3), CFS_KP(true, true, 6), CFS_KP(true, true, UM)}}};
#undef CFS_K
#undef CFS_KP
#undef CFS_KDET
    return (t.comb ? tab : ptab)[t.nt ? 1 : 0][t.offb ? 1 : 0][ui];
  }
  const void *tile_kernel() const {
    const TileVariant t = tile_variant();
    switch (t.block) {
    case 256: return pick_kernel<256>(t);
    case 512: return pick_kernel<512>(t);
    default: return pick_kernel<1024>(t);
    }
  }
  int launch_tiles(V *y, const V *x, hipStream_t st) {
    const void *k = tile_kernel();
    int rc = raise_lds_limit(k, device);
    if (rc) return rc;
    void *args[] = {(void *)&dev.tiles, (void *)&dev.gfirst, (void *)&dev.group_range,
                    (void *)&dev.slot_col, (void *)&dev.rowinfo, (void *)&dev.diag,
                    (void *)&dev.slice_meta, (void *)&dev.leadlane, (void *)&dev.vals,
                    (void *)&dev.slots,
                    (void *)&dev.cvals, (void *)&dev.crows, (void *)&dev.ccols,
                    (void *)&dev.fvals, (void *)&dev.frows, (void *)&dev.fcols,
                    (void *)&dev.strip, (void *)&dev.row_begin, (void *)&dev.lds_slots,
                    (void *)&x, (void *)&y, (void *)&dbg_buf, (void *)&dev_slot_exp};
    HIPCHK(hipLaunchKernel(k, dim3(P.ngroups), dim3(P.block_threads), args, lds_bytes, st));
    return 0;
  }

  int spmv_local(void *yv, const void *xv, void *sendv, hipStream_t st, int phases) override {
    V *y = (V *)yv;
    const V *x = (const V *)xv;
    if (P.tiles.empty()) return 0;
    if (phases & CFS_HIP_PHASE_TILES) {
      int rc = launch_tiles(y, x, st);
      if (rc) return rc;
    }
    // pack first: the exchange of a shard can then start while the local fold runs
    if ((phases & CFS_HIP_PHASE_PACK) && nsend > 0) {
      if (!sendv) return set_err(CFS_HIP_ERR_ARG, "shard has remote rows: send_buf required");
      hipLaunchKernelGGL((cfs_pack_kernel<V>), dim3((nsend + 255) / 256), dim3(256), 0,
                         st, (V *)sendv, (const V *)strip.p, (const int32_t *)send_ptr.p,
                         (const int32_t *)send_idx.p, nsend);
    }
    if ((phases & CFS_HIP_PHASE_FOLD) && nfold > 0)
      hipLaunchKernelGGL((cfs_fold_kernel<V>), dim3((nfold + 255) / 256), dim3(256), 0,
                         st, y, (const V *)strip.p, (const int4 *)fold_rec.p,
                         (const int32_t *)fold_idx.p, nfold);
    HIPCHK(hipGetLastError());
    return 0;
  }

  int set_recv(int nrecv, const int *rows) override {
    if (!cfs_plan::set_recv(P, nrecv, rows)) return set_err(CFS_HIP_ERR_ARG, P.error);
    int rc;
    rfold_rec = DevBuf();
    rfold_idx = DevBuf();
    {
      std::vector<int4> rec;
      std::vector<int32_t> rest;
      make_fold_records(P.rfold_row, P.rfold_ptr, P.rfold_idx, rec, rest);
      if ((rc = rfold_rec.upload(rec.data(), rec.size() * sizeof(int4)))) return rc;
      if ((rc = rfold_idx.upload(rest.data(), rest.size() * 4))) return rc;
    }
    nrfold = (int)P.rfold_row.size();
    return 0;
  }

  int recv_fold(void *yv, const void *recv, hipStream_t st) override {
    if (nrfold > 0)
      hipLaunchKernelGGL((cfs_fold_kernel<V>), dim3((nrfold + 255) / 256), dim3(256), 0,
                         st, (V *)yv, (const V *)recv, (const int4 *)rfold_rec.p,
                         (const int32_t *)rfold_idx.p, nrfold);
    HIPCHK(hipGetLastError());
    return 0;
  }

  void stats(cfs_hip_sym_stats *o) override {
    memset(o, 0, sizeof *o);
    const int64_t s = sizeof(V), rows_ = P.row_end - P.row_begin;
    o->n = P.n;
    o->row_begin = P.row_begin;
    o->row_end = P.row_end;
    o->value_bytes = (int)s;
    o->nnz_low = P.nnz_low;
    o->nnz_diag = P.nnz_diag;
    o->nnz_full = P.nnz_full;
    o->ntiles = (int)P.tiles.size();
    o->nslices = (int)nslices;
    o->max_slots_used = P.lds_slots;
    o->block_threads = P.block_threads;
    o->halo_slots = halo_slots;
    o->fold_rows = nfold;
    o->remote_vals = nsend;
    o->lds_bytes = (int64_t)lds_bytes;
    o->mirror_entries = mirror_entries;
    o->bytes_algorithmic = P.nnz_low * (4 + s) + rows_ * (4 + 3 * s);
    o->far_entries = far_entries;
    o->ngroups = P.ngroups;
    o->bytes_streamed = stream_len * s + slot_len * 2 + coo_len * (s + 4) + far_len * (2 * s + 6) +
                        rows_ * (4 + 3 * s) +
                        halo_slots * (4 + 2 * s) + rows_ * 8 /* slot_col, x, strip st */
                        + halo_slots * (4 + s)              /* fold: idx + strip ld  */
                        + (int64_t)(nfold + nsend) * (8 + 2 * s) + nslices * 16 +
                        (int64_t)P.tiles.size() * (int64_t)sizeof(Tile);
    o->device_bytes = (int64_t)(tiles.bytes + group_ptr.bytes + slot_col.bytes +
                                rowinfo.bytes + diag.bytes + slice_meta.bytes + leadlane.bytes + vals.bytes + cvals.bytes + crows.bytes + ccols.bytes +
                                fvals.bytes + frows.bytes + fcols.bytes + val_map.bytes + cval_map.bytes +
                                fval_map.bytes + diag_map.bytes +
                                slots.bytes + strip.bytes + fold_rec.bytes +
                                fold_idx.bytes + send_ptr.bytes + send_idx.bytes);
  }
  const std::vector<int32_t> &send_counts() override { return P.send_counts; }
  const std::vector<int32_t> &send_rows() override { return P.send_row; }
  int timeline(void *y, const void *x, unsigned long long *host, int cap, int *ng) override {
    *ng = P.ngroups;
    if (cap < P.ngroups * 8) return set_err(CFS_HIP_ERR_ARG, "buffer too small: need 8 words per group");
    DevBuf b;
    int rc = b.alloc((size_t)P.ngroups * 8 * sizeof(unsigned long long));
    if (rc) return rc;
    HIPCHK(hipMemset(b.p, 0, b.bytes));
    for (int it = 0; it < 3; it++) { // warm, then the recorded launch
      dbg_buf = it == 2 ? (unsigned long long *)b.p : nullptr;
      rc = spmv_local(y, x, nullptr, (hipStream_t)0, CFS_HIP_PHASE_TILES);
      dbg_buf = nullptr;
      if (rc) return rc;
    }
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host, b.p, b.bytes, hipMemcpyDeviceToHost));
    return 0;
  }
  // per persistent group, kCfsGroupFeatures words (cfs_hip_sym_debug_group_features)
  int group_features(long long *out, int cap, int *ng) override {
    *ng = P.ngroups;
    if (cap < P.ngroups * CFS_HIP_GROUP_FEATURES)
      return set_err(CFS_HIP_ERR_ARG, "buffer too small");
    const int T = (int)P.tiles.size();
    for (int sl = 0; sl < P.ngroups; sl++) { // in launch-slot order
      const int g = (int)P.launch_order.size() == P.ngroups ? P.launch_order[sl] : sl;
      long long *o = out + (size_t)sl * CFS_HIP_GROUP_FEATURES;
      for (int k = 0; k < CFS_HIP_GROUP_FEATURES; k++) o[k] = 0;
      for (int ti = P.group_ptr[g]; ti < P.group_ptr[g + 1]; ti++) {
        const Tile &t = P.tiles[ti];
        o[0] += 1;
        o[1] += t.nown;
        o[2] += t.nvrows;
        o[3] += t.nslices;
        o[4] += ti < (int)P.tile_rounds.size() ? P.tile_rounds[ti] : 0;
        o[5] += (ti + 1 < T ? P.tiles[ti + 1].nnz_off : stream_len) - t.nnz_off;
        o[6] += (ti + 1 < T ? P.tiles[ti + 1].sl_off : slot_len) - t.sl_off;
        o[7] += t.ncoo;
        o[8] += t.nslots - t.nown;
        o[9] += t.nslots;
      }
    }
    return 0;
  }
  int update_values(const void *values_dev, long long nnz, hipStream_t st) override {
    if (!has_value_map)
      return set_err(CFS_HIP_ERR_ARG, "handle was created without CFS_HIP_FLAG_KEEP_VALUE_MAP");
    if (P.deterministic)
      return set_err(CFS_HIP_ERR_UNSUPPORTED, "deterministic handle: its fixed-point scale depends on the values");
    if (nnz != nnz_caller) return set_err(CFS_HIP_ERR_ARG, "value count differs from the matrix the handle was built from");
    const V *src = (const V *)values_dev;
    auto go = [&](DevBuf &dst, DevBuf &map) {
      const long long cnt = (long long)(map.bytes / 4);
      if (cnt <= 0) return;
      const int grid = (int)std::min<long long>((cnt + 255) / 256, 256 * 16);
      hipLaunchKernelGGL((cfs_value_scatter_kernel<V>), dim3(grid), dim3(256), 0, st, (V *)dst.p,
                         (const int32_t *)map.p, src, cnt);
    };
    go(vals, val_map);
    go(cvals, cval_map);
    go(fvals, fval_map);
    go(diag, diag_map);
    HIPCHK(hipGetLastError());
    values_epoch += 1;
    return 0;
  }
  int diagonal(void *d_dev, hipStream_t st) override {
    const int T = (int)P.tiles.size();
    if (T == 0) return 0;
    int window = 1; // own rows of the tallest tile
    for (const Tile &t : P.tiles) window = std::max(window, (int)t.nown);
    const void *k = (const void *)cfs_diag_gather_kernel<V>;
    int rc = raise_lds_limit(k, device); // (a window of 1 024-thread tiles can exceed the 64 KiB default)
    if (rc) return rc;
    hipLaunchKernelGGL((cfs_diag_gather_kernel<V>), dim3(std::min(T, 4096)), dim3(256), (size_t)window * sizeof(V), st,
                       (V *)d_dev, dev.tiles, T, dev.slot_col, dev.rowinfo, dev.diag, (int)P.row_begin,
                       (int)(P.row_end - P.row_begin), window);
    HIPCHK(hipGetLastError());
    return 0;
  }
  int block_diagonal(void *blocks_dev, int bs, hipStream_t st) override {
    if (P.nranks != 1 || P.row_begin != 0 || P.row_end != P.n)
      return set_err(CFS_HIP_ERR_UNSUPPORTED, "block diagonal: a handle of the whole matrix, not a shard (blocks straddle "
                                              "the row splits)");
    if (bs == 1) return diagonal(blocks_dev, st); // the diagonal itself: every word written exactly once
    const long long nb = ((long long)P.n + bs - 1) / bs;
    HIPCHK(hipMemsetAsync(blocks_dev, 0, (size_t)nb * bs * bs * sizeof(V), st));
    const int T = (int)P.tiles.size();
    if (T == 0) return 0;
    int window = 1; // own rows of the tallest tile
    for (const Tile &t : P.tiles) window = std::max(window, (int)t.nown);
    const void *k = (const void *)cfs_block_gather_kernel<V>;
    int rc = raise_lds_limit(k, device);
    if (rc) return rc;
    hipLaunchKernelGGL((cfs_block_gather_kernel<V>), dim3(std::min(T, 4096)), dim3(256), (size_t)window * sizeof(V), st,
                       (V *)blocks_dev, dev.tiles, T, dev, (int)P.n, bs, window);
    HIPCHK(hipGetLastError());
    return 0;
  }
  int n() override { return P.n; }
  int rows() override { return P.row_end - P.row_begin; }
};

#include "cfs_devplan.hpp" // tune() on the GPU (needs SymMatrix and cfs_value_scatter_kernel)
#include "cfs_csr.hpp"     // the general CSR path: kernels, handle, create / launch
#include "cfs_solver.hpp"  // conjugate gradients on resident vectors (a solver-style caller)
#include "cfs_solver_mixed.hpp" // the same recurrence on an fp32 handle, the solution and true residuals in fp64
#include "cfs_solver_minres.hpp" // MINRES for symmetric indefinite and shifted systems, the same launch layout
#include "cfs_solver_eigs.hpp" // thick-restart Lanczos for extreme eigenpairs: tall-skinny algebra against a resident basis
#include "cfs_solver_lobpcg.hpp" // LOBPCG for the smallest eigenpairs with the PCG preconditioners: a small SYRK per iteration
#include "cfs_solver_cheb.hpp" // a Chebyshev polynomial in M^-1 A as the PCG preconditioner, and the power method for its bound
#include "cfs_solver_amg.hpp" // an aggregation multigrid V-cycle as the PCG preconditioner: the hierarchy on the host, the cycle on the device
#include "cfs_multi.hpp"   // one host thread, N devices: MultiSym, its create and cfs_hip_sym_multi_*


// ---------------------------------------------------------------------------
// C ABI (every function below is declared extern "C" in cfs_hip.h)
// ---------------------------------------------------------------------------

int cfs_hip_abi_version(void) { return CFS_HIP_ABI_VERSION; }
const char *cfs_hip_last_error(void) { return cfs_rt::last_error().c_str(); }

int cfs_hip_device_count(int *count) {
  if (!count) return set_err(CFS_HIP_ERR_ARG, "count is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return set_err(CFS_HIP_ERR_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = c;
  return 0;
}

// Make `device` the calling thread's current device and the home of the
// synchronous entry points.  Contexts (streams) of other devices stay alive:
// handles created on them keep working.
int cfs_hip_init(int device) { return cfs_rt::bind_home(device); }

int cfs_hip_current_device(int *device) {
  if (!device) return set_err(CFS_HIP_ERR_ARG, "device is NULL");
  int rc = ensure_init();
  if (rc) return rc;
  *device = cfs_rt::rt().home.load();
  return 0;
}

// 1 once a home device is bound (cfs_hip_init, or the first entry point that needed one);
// never initialises anything itself
int cfs_hip_runtime_bound(void) { return cfs_rt::rt().home.load() >= 0 ? 1 : 0; }

int cfs_hip_default_stream(void **stream) {
  int rc = ensure_init();
  if (rc) return rc;
  *stream = (void *)cfs_rt::home_stream();
  return 0;
}

int cfs_hip_synchronize(void *stream) {
  int rc = ensure_init();
  if (rc) return rc;
  if (stream) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
  }
  // NULL: the library streams of the synchronous entry points, on every device
  // a handle of this process lives on (a matrix sharded over N GPUs by the C++
  // surface runs on N of them)
  for (int d = 0; d < cfs_rt::kMaxDevices; d++) {
    hipStream_t st;
    {
      std::lock_guard<std::mutex> lk(cfs_rt::rt().mu);
      st = cfs_rt::rt().ctx[d].stream;
    }
    if (!st) continue;
    DeviceGuard g(d);
    HIPCHK(hipStreamSynchronize(st));
  }
  return 0;
}

int cfs_hip_alloc(size_t bytes, int kind, void **out) {
  if (!out) return set_err(CFS_HIP_ERR_ARG, "out is NULL");
  int rc = ensure_init();
  if (rc) return rc;
  if (bytes == 0) bytes = 64;
  if (kind == CFS_HIP_MEM_DEVICE) {
    DeviceGuard g(cfs_rt::rt().home.load());
    HIPCHK(hipMalloc(out, bytes));
  } else if (kind == CFS_HIP_MEM_PINNED) {
    return cfs_rt::pinned().alloc(bytes, out);
  } else {
    return set_err(CFS_HIP_ERR_ARG, "unknown memory kind");
  }
  return 0;
}

int cfs_hip_free(void *p, int kind) {
  if (!p) return 0;
  if (kind == CFS_HIP_MEM_DEVICE) {
    // (hipFree finds the owning device itself; the guard keeps the calling thread's
    // current device what it was on runtimes that switch to the owner)
    const cfs_rt::PtrInfo pi = cfs_rt::classify(p);
    DeviceGuard g(pi.device ? pi.dev : -1);
    HIPCHK(hipFree(p));
  }
  else if (kind == CFS_HIP_MEM_PINNED) return cfs_rt::pinned().release(p);
  else return set_err(CFS_HIP_ERR_ARG, "unknown memory kind");
  return 0;
}

int cfs_hip_pinned_owns(const void *p) { return p && cfs_rt::pinned().owns(p) ? 1 : 0; }

int cfs_hip_pinned_pool_stats(size_t *live_blocks, size_t *spare_blocks, size_t *spare_bytes) {
  size_t a = 0, b = 0, c = 0;
  cfs_rt::pinned().stats(&a, &b, &c);
  if (live_blocks) *live_blocks = a;
  if (spare_blocks) *spare_blocks = b;
  if (spare_bytes) *spare_bytes = c;
  return 0;
}

int cfs_hip_memcpy(void *dst, const void *src, size_t bytes, int dir) {
  int rc = ensure_init();
  if (rc) return rc;
  hipMemcpyKind k = dir == CFS_HIP_H2D   ? hipMemcpyHostToDevice
                    : dir == CFS_HIP_D2H ? hipMemcpyDeviceToHost
                                         : hipMemcpyDeviceToDevice;
  if ((rc = cfs_hip_synchronize(nullptr))) return rc; // pending SpMVs on resident vectors
  HIPCHK(hipMemcpy(dst, src, bytes, k));
  return 0;
}

int cfs_hip_memset(void *dst, int value, size_t bytes) {
  if (!dst) return set_err(CFS_HIP_ERR_ARG, "dst is NULL");
  int rc = ensure_init();
  if (rc) return rc;
  const cfs_rt::PtrInfo pi = cfs_rt::classify(dst);
  DeviceGuard g(pi.device ? pi.dev : -1);
  if ((rc = cfs_hip_synchronize(nullptr))) return rc; // pending SpMVs on resident vectors
  HIPCHK(hipMemset(dst, value, bytes));
  return 0;
}

// what a refusal of the schedule builder means to the caller.  UNSUPPORTED is
// reserved for matrices the tile schedule does not cover (a row denser than an LDS
// window, 16-/25-/31-bit offsets exhausted): src/csr.cpp then binds the general CSR
// kernel.  Bad arguments, the mirror refusals of a shard and builder bugs get codes
// of their own -- they must never turn into a quietly slower path.
static int plan_error_code(const std::string &e) {
  if (e.rfind("mirror:", 0) == 0) return CFS_HIP_ERR_MIRROR;
  if (e.rfind("internal:", 0) == 0) return CFS_HIP_ERR_INTERNAL;
  if (e.rfind("bad ", 0) == 0 || e.rfind("block_threads", 0) == 0) return CFS_HIP_ERR_ARG;
  return CFS_HIP_ERR_UNSUPPORTED;
}

static cfs_plan::Options to_opts(const cfs_hip_options *o) {
  cfs_plan::Options r;
  if (o) {
    r.max_slots = o->max_slots;
    r.max_tile_nnz = o->max_tile_nnz;
    r.block_threads = o->block_threads;
    r.flags = o->flags;
    r.reorder = !(o->flags & CFS_HIP_FLAG_NO_REORDER);
    if (o->flags & CFS_HIP_FLAG_FORCE_CLUSTER) r.force_order = 2;
    if (o->flags & CFS_HIP_FLAG_SHARD_EXCHANGE) r.mirror_offblock = false;
    if (o->flags & CFS_HIP_FLAG_HYB) r.hyb = true;
    if (o->flags & CFS_HIP_FLAG_DETERMINISTIC) r.deterministic = true;
    if (o->flags & CFS_HIP_FLAG_KEEP_VALUE_MAP) r.keep_value_map = true;
  }
  // developer knobs (like CFS_HIP_MAX_SLOTS): far threshold, HYB on / off
  if (const char *e = getenv("CFS_HIP_FAR_USES"))
    if (atoi(e) > 0) r.far_uses = atoi(e);
  if (const char *e = getenv("CFS_HIP_HYB")) r.hyb = atoi(e) != 0;
  if (const char *e = getenv("CFS_HIP_COST_MODEL")) r.cost_model = atoi(e) != 0;
  if (const char *e = getenv("CFS_HIP_COMBINE")) r.combine_siblings = atoi(e) != 0;
  if (const char *e = getenv("CFS_HIP_DETERMINISTIC")) r.deterministic = atoi(e) != 0;
  if (r.deterministic && r.block_threads == 256) r.block_threads = 512; // 512 / 1 024 threads
  if (o && (o->flags & CFS_HIP_FLAG_NO_HYB)) r.hyb = false;
  r.count_far = !r.hyb && !(o && (o->flags & (CFS_HIP_FLAG_NO_CALIBRATE | CFS_HIP_FLAG_NO_HYB)));
  // tuning knob for callers that cannot pass options (the C++ surface): LDS slots
  // per tile, like CFS_NUM_THREADS for the reference's partitions
  if (r.max_slots <= 0) {
    const char *e = getenv("CFS_HIP_MAX_SLOTS");
    if (e && atoi(e) > 0) r.max_slots = atoi(e);
  }
  // developer knob (tools/calib_probe.py): relative cost share of every persistent group
  if (const char *e = getenv("CFS_HIP_GROUP_SHARE_FILE"))
    if (FILE *f = fopen(e, "r")) {
      double v;
      while (fscanf(f, "%lf", &v) == 1) r.group_share.push_back(v);
      fclose(f);
    }
  return r;
}

// how many workgroups of the tile kernel are co-resident on a CU for the LDS
// budget the options ask for: the persistent grid is sized to exactly one
// resident wave of workgroups (a workgroup that has to wait for a slot would
// run as a second round and double the launch time)
template <typename V, int BLOCK> static int residency_one(size_t lds, int *nb, bool det = false) {
  const void *k = det ? (const void *)cfs_sym_tile_kernel<V, (BLOCK < 512 ? 512 : BLOCK), 0, true, true,
                                                          cfs_plan::kSlotsPerThread, true>
                      : (const void *)cfs_sym_tile_kernel<V, BLOCK, 0, true, true, cfs_plan::kSlotsPerThread>;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  int rc = raise_lds_limit(k, dev);
  if (rc) return rc;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, k, BLOCK, lds));
  return 0;
}
template <typename V> static int query_residency(cfs_plan::Options &po) {
  // the window the plan builder will allow (same rule: cfs_plan::chunk_layout)
  const cfs_plan::ChunkLayout L = cfs_plan::chunk_layout<V>(1 << 30, po);
  const int block = L.block;
  const int slot_bytes = cfs_plan::slot_lds_bytes<V>(po.deterministic);
  const size_t lds = (size_t)((L.max_slots + 63) / 64 * 64) * slot_bytes;
  int nb = 0, rc;
  switch (block) {
  case 256: rc = residency_one<V, 256>(lds, &nb); break;
  case 512: rc = residency_one<V, 512>(lds, &nb, po.deterministic); break;
  case 1024: rc = residency_one<V, 1024>(lds, &nb, po.deterministic); break;
  default: return 0; // build_plan reports the bad block size
  }
  if (rc) return rc;
  hipDeviceProp_t prop;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  po.wg_per_cu = nb > 0 ? nb : 1;
  po.num_cus = prop.multiProcessorCount;
  return 0;
}

template <typename V>
static int sym_create(int n, const int *rowptr, const int *colind, const V *values,
                      int nranks, int rank, const int *row_splits,
                      const cfs_hip_options *opt, cfs_hip_sym_t *out) {
  if (!out) return set_err(CFS_HIP_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (n < 0 || !rowptr || (n > 0 && rowptr[n] > 0 && (!colind || !values)))
    return set_err(CFS_HIP_ERR_ARG, "null CSR array");
  if (nranks < 1 || rank < 0 || rank >= nranks)
    return set_err(CFS_HIP_ERR_ARG, "bad rank / nranks");
  if (nranks > 1 && !row_splits) return set_err(CFS_HIP_ERR_ARG, "row_splits required");
  cfs_plan::PhaseTimer ct;
  int rc = ensure_init();
  if (rc) return rc;
  int cur_dev = 0;
  HIPCHK(hipGetDevice(&cur_dev));
  std::unique_ptr<SymMatrix<V>> m(new SymMatrix<V>());
  m->value_bytes = (int)sizeof(V);
  m->device = cur_dev;
  cfs_plan::Options po = to_opts(opt);
  if ((rc = query_residency<V>(po))) return rc;
  ct.lap("create: runtime + kernel residency");
  // kept until the window-shape step below has had its chance to reuse it
  cfs_plan::ScheduleSpace<V> space;
  const bool want_tuning = !(opt && (opt->flags & CFS_HIP_FLAG_NO_CALIBRATE));
  // the schedule: built on the GPU (cfs_devplan.hpp) when the options are covered, else -- and
  // whenever the device builder hands over -- by the host builder + upload
  const bool host_plan = (opt && (opt->flags & CFS_HIP_FLAG_HOST_PLAN)) ||
                         (getenv("CFS_HIP_DEVICE_PLAN") && atoi(getenv("CFS_HIP_DEVICE_PLAN")) == 0);
  auto build_handle = [&](SymMatrix<V> *h, cfs_plan::Options &o, cfs_plan::ScheduleSpace<V> *sp) -> int {
    h->nnz_caller = rowptr[n];
    if (!host_plan) {
      std::string why;
      const int r2 = cfs_dev::build<V>(n, rowptr, colind, values, nranks, rank,
                                       nranks > 1 ? row_splits : nullptr, o, *h, sp, why);
      if (r2 == 0) return h->adopt_device_schedule(); // (the builder's temporaries are gone by now)
      if (r2 < 0) return r2;
      if (getenv("CFS_PLAN_VERBOSE")) fprintf(stderr, "[cfs_hip] device builder hands over: %s\n", why.c_str());
      h->device_built = false;
      h->plan_note = why.empty() ? "handed over" : why;
    }
    if (!cfs_plan::build_plan<V>(n, rowptr, colind, values, nranks, rank, nranks > 1 ? row_splits : nullptr, o,
                                 h->P, sp))
      return set_err(plan_error_code(h->P.error), h->P.error);
    return h->upload();
  };
  rc = build_handle(m.get(), po, want_tuning ? &space : nullptr);
  ct.lap("create: schedule (build + upload)");
  if (rc) return rc;
  // ---- window shape (Tuning::Aggressive; CFS_HIP_FLAG_NO_CALIBRATE skips it) -------
  // Default: 512 threads, 4 992 slots, two workgroups per CU.  A matrix that is
  // scheduled in clustered order (compact 3-D tiles) can be faster with ONE
  // workgroup of 1 024 threads and a window twice the size per CU -- half as many,
  // larger tiles, a quarter fewer halo slots, a shorter fold (Flan stand-in fp64:
  // 0.122 -> 0.116 ms per SpMV; fp32, ldoor, pwtk, Queen: no gain or a loss).
  // Both schedules are built and timed; the faster one is kept.
  const bool tuning = !(opt && (opt->flags & CFS_HIP_FLAG_NO_CALIBRATE)) &&
                      m->P.nnz_low >= (int64_t)2000000;
  // a measured step: build the alternative schedule, time ten SpMVs of each
  // (interleaved, best of three), keep the faster one
  DevBuf xb, yb;
  auto time_spmv = [&](SymMatrix<V> *h, float *ms) -> int {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
    int r2 = 0;
    for (int it = 0; it < 3 && !r2; it++) r2 = h->spmv_local(yb.p, xb.p, nullptr, (hipStream_t)0, 3);
    (void)hipEventRecord(a, (hipStream_t)0);
    for (int it = 0; it < 10 && !r2; it++) r2 = h->spmv_local(yb.p, xb.p, nullptr, (hipStream_t)0, 3);
    (void)hipEventRecord(b, (hipStream_t)0);
    if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(ms, a, b) != hipSuccess) r2 = -1;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return r2;
  };
  auto ensure_xy = [&]() -> int {
    if (xb.p) return 0;
    int r2;
    if ((r2 = xb.alloc((size_t)n * sizeof(V))) || (r2 = yb.alloc((size_t)m->rows() * sizeof(V)))) return r2;
    (void)hipMemset(xb.p, 0x3f, xb.bytes); // small positive values
    return 0;
  };
  // which instantiation of the tile kernel (sibling-combined atomics or plain) a handle
  // launches: same schedule, same arrays -- time ten SpMVs of each, three times
  auto choose_kernel = [&](SymMatrix<V> *h) -> int {
    if (!h->combine_ok || h->combine_forced) return 0;
    int r2 = ensure_xy();
    if (r2) return r2;
    const bool dflt = h->combine; // the size rule's choice (upload()): kept unless the other
    float t[2] = {1e30f, 1e30f};  // instantiation is clearly -- 3 %, best of three -- faster
    for (int round = 0; round < 3; round++)
      for (int c = 0; c < 2; c++) {
        float ms = 0;
        h->combine = c == 1;
        if (time_spmv(h, &ms)) {
          h->combine = dflt;
          return 0;
        }
        t[c] = std::min(t[c], ms);
      }
    h->combine = t[dflt ? 0 : 1] < 0.97f * t[dflt ? 1 : 0] ? !dflt : dflt;
    if (getenv("CFS_PLAN_VERBOSE"))
      fprintf(stderr, "[cfs_hip] tile kernel: plain %.1f us, sibling-combined atomics %.1f us\n", t[0] * 100.0,
              t[1] * 100.0);
    return 0;
  };
  auto try_alternative = [&](cfs_plan::Options &po2, cfs_plan::ScheduleSpace<V> *sp,
                             const char *what, int forced = -1) -> int {
    {
      int r2 = ensure_xy();
      if (r2) return r2;
    }
    std::unique_ptr<SymMatrix<V>> alt(new SymMatrix<V>());
    alt->value_bytes = (int)sizeof(V);
    alt->device = cur_dev;
    alt->nnz_caller = rowptr[n];
    float t_def = 0, t_alt = 0;
    bool ok = query_residency<V>(po2) == 0 && build_handle(alt.get(), po2, sp) == 0 && choose_kernel(alt.get()) == 0;
    for (int round = 0; ok && round < 3; round++) {
      float a = 0, b = 0;
      ok = time_spmv(m.get(), &a) == 0 && time_spmv(alt.get(), &b) == 0;
      t_def = round == 0 ? a : std::min(t_def, a);
      t_alt = round == 0 ? b : std::min(t_alt, b);
    }
    if (getenv("CFS_PLAN_VERBOSE"))
      fprintf(stderr, "[cfs_hip] %s: current %.1f us, alternative %.1f us%s\n", what, t_def * 100.0,
              t_alt * 100.0, ok ? "" : " (alternative not built)");
    // (CFS_HIP_KEEP_ALT=1: developer knob -- keep the alternative whatever the clock says,
    // so that each of the schedules tune() may end up with can be profiled on any box)
    const char *force = getenv("CFS_HIP_KEEP_ALT");
    if (force && atoi(force) != 0) forced = 1;
    if (ok && forced != 0 && (t_alt < 0.99f * t_def || forced == 1)) {
      m = std::move(alt);
      po = po2;
    }
    return 0;
  };
  if (tuning && (rc = choose_kernel(m.get()))) return rc;
  // (natural-order schedules are tried too: a 1/8 row block of the Flan stand-in runs 11 %
  // faster with 256 workgroups of 1 024 threads -- a third less halo, half as many window
  // phases per CU -- while pwtk, ldoor and Queen stay with the default)
  if (tuning && po.block_threads == 0 && po.max_slots == 0) {
    cfs_plan::Options po2 = po;
    po2.block_threads = 1024;
    po2.max_slots = 2 * cfs_plan::kDefaultSlots;
    // (CFS_HIP_SHAPE=512|1024: developer knob -- the profiler passes of one evidence set
    // must run the schedule its bench line ran, whatever the clock says under the profiler)
    int forced = -1;
    if (const char *e = getenv("CFS_HIP_SHAPE")) forced = atoi(e) == 1024 ? 1 : (atoi(e) == 512 ? 0 : -1);
    if ((rc = try_alternative(po2, &space, "window shape 512 x 2 per CU vs 1024 x 1", forced))) return rc;
  }
  // ---- HYB by measurement (Format::sss, Tuning::Aggressive) --------------------------
  // A halo column that its tile uses once costs a slot, a slot-table entry, an x
  // gather, a strip store and a fold entry for one nonzero; as a FAR entry the nonzero
  // is stored twice and gathers x from L2.  Worth trying when such columns are a
  // noticeable share of the matrix (ldoor stand-in: 6 % of the stored nonzeros, halo
  // 2.55M -> 1.16M slots, 71 -> 66 us per SpMV; Flan, pwtk stand-ins: < 0.1 %, not tried).
  const bool may_hyb = !(opt && (opt->flags & (CFS_HIP_FLAG_NO_HYB | CFS_HIP_FLAG_HYB))) && !po.hyb;
  if (tuning && may_hyb && m->P.far_candidates * 33 >= m->P.nnz_low) {
    cfs_plan::Options po2 = po;
    po2.hyb = true;
    int forced = -1; // CFS_HIP_TAKE_HYB=1|0: keep / drop the alternative whatever the clock says (tests)
    if (const char *e = getenv("CFS_HIP_TAKE_HYB")) forced = atoi(e) != 0 ? 1 : 0;
    // (the kept upload / schedule space of the builds above serves this one too)
    if ((rc = try_alternative(po2, &space, "tile format vs HYB (far entries apart)", forced))) return rc;
  }
  space.drop(); // release the schedule-space matrix / the kept upload
  m->ablate_mode = opt ? (opt->flags & CFS_HIP_FLAG_ABLATE_MASK) : 0;
  m->build_flags = opt ? opt->flags : 0;
  m->num_cus = po.num_cus;
  *out = m.release();
  ct.lap("create: measured alternatives");
  return 0;
}

int cfs_hip_sym_create_f64(int n, const int *rowptr, const int *colind, const double *values,
                           const cfs_hip_options *opt, cfs_hip_sym_t *out) {
  return sym_create<double>(n, rowptr, colind, values, 1, 0, nullptr, opt, out);
}
int cfs_hip_sym_create_f32(int n, const int *rowptr, const int *colind, const float *values,
                           const cfs_hip_options *opt, cfs_hip_sym_t *out) {
  return sym_create<float>(n, rowptr, colind, values, 1, 0, nullptr, opt, out);
}
int cfs_hip_sym_create_shard_f64(int n, const int *rowptr, const int *colind,
                                 const double *values, int nranks, int rank,
                                 const int *row_splits, const cfs_hip_options *opt,
                                 cfs_hip_sym_t *out) {
  return sym_create<double>(n, rowptr, colind, values, nranks, rank, row_splits, opt, out);
}
int cfs_hip_sym_create_shard_f32(int n, const int *rowptr, const int *colind,
                                 const float *values, int nranks, int rank,
                                 const int *row_splits, const cfs_hip_options *opt,
                                 cfs_hip_sym_t *out) {
  return sym_create<float>(n, rowptr, colind, values, nranks, rank, row_splits, opt, out);
}

int cfs_hip_sym_balanced_splits(int n, const int *rowptr, const int *colind, int nranks,
                                int *row_splits) {
  if (n < 0 || !rowptr || !row_splits || nranks < 1)
    return set_err(CFS_HIP_ERR_ARG, "bad argument");
  cfs_plan::balanced_splits(n, rowptr, colind, nranks, row_splits);
  return 0;
}

int cfs_hip_sym_destroy(cfs_hip_sym_t h) {
  delete h;
  return 0;
}

// the async entry points take device pointers on the caller's stream; the
// placement of a (y, x) pair is checked once (hipPointerGetAttributes costs more
// than the launch): vectors on another device than the matrix would fault or, with
// peer access, silently run over the fabric
static int check_placement(cfs_hip_sym_t h, const void *y, const void *x) {
  if (h->ok_x == x && h->ok_y == y) return 0;
  const cfs_rt::PtrInfo xi = cfs_rt::classify(x), yi = cfs_rt::classify(y);
  if (!xi.device || !yi.device)
    return set_err(CFS_HIP_ERR_ARG, "async entry points need device pointers (use cfs_hip_sym_spmv)");
  if (xi.dev != h->device || yi.dev != h->device)
    return set_err(CFS_HIP_ERR_ARG, "x / y live on device " +
                                        std::to_string(xi.dev != h->device ? xi.dev : yi.dev) +
                                        ", the matrix on device " + std::to_string(h->device));
  h->ok_x = x;
  h->ok_y = y;
  return 0;
}

int cfs_hip_sym_spmv_async(cfs_hip_sym_t h, void *y, const void *x, void *stream) {
  if (!h || !y || !x) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (!h->send_rows().empty())
    return set_err(CFS_HIP_ERR_ARG, "sharded handle: use cfs_hip_sym_spmv_local_async");
  int rc = check_placement(h, y, x);
  if (rc) return rc;
  DeviceGuard g(h->device);
  return h->spmv_local(y, x, nullptr, (hipStream_t)stream);
}

// ---- the solve entry points ------------------------------------------------------------------------
// What each of them checks of its (u, b) or (z, r) pair, in one order.  check_solve_args: what needs no look at the
// handle -- null, the outputs zeroed, u != b, 16-byte alignment, tol / maxiter (tol = nullptr: the entry point has
// none).  Then the entry point's own arguments.  Then check_solve_handle: a handle of the whole matrix, on one device
// where that is required, the placement of the pair, and ok_x = ok_y = nullptr (the iteration's own vectors are
// library memory on the handle's device).
//   who: the prefix of the refusals;  inner: that of the alignment and tolerance refusals (cfs_hip_sym_pcg and
//   _pcg_block have always answered those with cg's);  pair: "u and b" / "z and r"
static int check_solve_args(const char *who, const char *inner, const char *pair, bool any_null, const void *u, const void *b,
                            const double *tol, int maxiter, int *iterations, int *replacements, double *relres,
                            const char *null_text = "null argument") {
  if (any_null) return set_err(CFS_HIP_ERR_ARG, null_text);
  if (iterations) *iterations = 0;
  if (replacements) *replacements = 0;
  if (relres) *relres = 0.0;
  if (u == b) return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": " + pair + " must be different vectors");
  if ((((uintptr_t)u) | ((uintptr_t)b)) & 15) return set_err(CFS_HIP_ERR_ARG, std::string(inner) + ": " + pair + " must be 16-byte aligned");
  if (tol && (maxiter < 0 || !(*tol >= 0.0))) return set_err(CFS_HIP_ERR_ARG, std::string(inner) + ": bad tolerance / iteration limit");
  return 0;
}
static std::string not_a_shard(const char *who) { return std::string(who) + ": a handle of the whole matrix, not a shard"; }
// the refusal of a multi-device handle where node blocks are used ("": block_rows < 2, any handle of the whole matrix)
static std::string blocks_on_one_device(const char *who, int block_rows) {
  if (block_rows < 2) return "";
  return std::string(who) + ": block Jacobi needs the whole matrix on one device (blocks straddle the row splits of a multi-device handle)";
}
// shard: the refusal of a handle that is not of the whole matrix (rows_too: a row block without sends counts);
// one_device: the refusal of a multi-device handle, or "" where one is accepted
static int check_whole_matrix(cfs_hip_sym_t h, const std::string &shard, bool rows_too, const std::string &one_device) {
  if (!h->send_rows().empty() || (rows_too && h->rows() != h->n())) return set_err(CFS_HIP_ERR_UNSUPPORTED, shard);
  int ngpus = 1;
  if (!one_device.empty() && cfs_hip_sym_num_gpus(h, &ngpus) == 0 && ngpus != 1) return set_err(CFS_HIP_ERR_UNSUPPORTED, one_device);
  return 0;
}
static int check_solve_handle(cfs_hip_sym_t h, const void *u, const void *b, const std::string &shard, bool rows_too,
                              const std::string &one_device) {
  int rc = check_whole_matrix(h, shard, rows_too, one_device);
  if (rc || (rc = check_placement(h, u, b))) return rc;
  h->ok_x = h->ok_y = nullptr;
  return 0;
}

static bool block_rows_ok(int bs) { return bs == 1 || bs == 2 || bs == 3 || bs == 4 || bs == 6; }
// f(V(), std::integral_constant<int, BS>()) for the handle's value type and a stored M^-1 of 0 (none), 1 (Jacobi) or
// node blocks of 2, 3, 4 or 6 rows: the BS of cfs_solver::Precond
template <class F> static int with_precond(int value_bytes, int bs, F &&f) {
  return cfs_rt::with_value_type(value_bytes, [&](auto v) {
    switch (bs) {
    case 0: return f(v, std::integral_constant<int, 0>());
    case 1: return f(v, std::integral_constant<int, 1>());
    case 2: return f(v, std::integral_constant<int, 2>());
    case 3: return f(v, std::integral_constant<int, 3>());
    case 4: return f(v, std::integral_constant<int, 4>());
    default: return f(v, std::integral_constant<int, 6>());
    }
  });
}
// the handles an entry point with a stored M^-1 accepts: those of cfs_hip_sym_pcg (0, 1) or of cfs_hip_sym_pcg_block
static int check_precond_handle(cfs_hip_sym_t h, int block_rows, const char *who) {
  return check_whole_matrix(h, not_a_shard(who), true, blocks_on_one_device(who, block_rows));
}

// cfs_hip_sym_cg (block_rows 0), _pcg (1) and _pcg_block (2, 3, 4, 6) behind their checks: one code path
static int run_cg(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int block_rows, double tol, int maxiter, int check_every,
                  int *iterations, double *relres, void *stream) {
  DeviceGuard g(h->device);
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::cg<decltype(v), decltype(bs)::value>(h, u_dev, b_dev, tol, maxiter, check_every, iterations, relres,
                                                            (hipStream_t)stream);
  });
}

int cfs_hip_sym_cg(cfs_hip_sym_t h, void *u_dev, const void *b_dev, double tol, int maxiter, int check_every,
                   int *iterations, double *relres, void *stream) {
  int rc = check_solve_args("cg", "cg", "u and b", !h || !u_dev || !b_dev, u_dev, b_dev, &tol, maxiter, iterations, nullptr, relres);
  if (rc || (rc = check_solve_handle(h, u_dev, b_dev,
                                     "cg: a handle of the whole matrix (a loop over shards of several processes: cfs_spmv_amd/solver.py)",
                                     false, "")))
    return rc;
  return run_cg(h, u_dev, b_dev, 0, tol, maxiter, check_every, iterations, relres, stream);
}

int cfs_hip_sym_pcg(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int precond, double tol, int maxiter,
                    int check_every, int *iterations, double *relres, void *stream) {
  if (precond == CFS_HIP_PRECOND_NONE) // the plain iteration: the same code path, the same bits
    return cfs_hip_sym_cg(h, u_dev, b_dev, tol, maxiter, check_every, iterations, relres, stream);
  int rc = check_solve_args("pcg", "cg", "u and b", !h || !u_dev || !b_dev, u_dev, b_dev, &tol, maxiter, iterations, nullptr, relres);
  if (rc) return rc;
  if (precond != CFS_HIP_PRECOND_JACOBI) return set_err(CFS_HIP_ERR_ARG, "pcg: unknown preconditioner " + std::to_string(precond));
  if ((rc = check_solve_handle(h, u_dev, b_dev, not_a_shard("pcg"), false, ""))) return rc;
  return run_cg(h, u_dev, b_dev, 1, tol, maxiter, check_every, iterations, relres, stream);
}

int cfs_hip_sym_diagonal_async(cfs_hip_sym_t h, void *d_dev, void *stream) {
  if (!h || !d_dev) return set_err(CFS_HIP_ERR_ARG, "null argument");
  const cfs_rt::PtrInfo di = cfs_rt::classify(d_dev);
  if (!di.device) return set_err(CFS_HIP_ERR_ARG, "cfs_hip_sym_diagonal_async needs a device pointer");
  if (di.dev != h->device)
    return set_err(CFS_HIP_ERR_ARG, "d lives on device " + std::to_string(di.dev) + ", the matrix on device " +
                                        std::to_string(h->device));
  DeviceGuard g(h->device);
  return h->diagonal(d_dev, (hipStream_t)stream);
}

// the output of the two block entry points: a device pointer on the handle's device
static int check_block_out(cfs_hip_sym_t h, const void *p, const char *who) {
  const cfs_rt::PtrInfo di = cfs_rt::classify(p);
  if (!di.device) return set_err(CFS_HIP_ERR_ARG, std::string(who) + " needs a device pointer");
  if (di.dev != h->device)
    return set_err(CFS_HIP_ERR_ARG, "the blocks live on device " + std::to_string(di.dev) + ", the matrix on device " +
                                        std::to_string(h->device));
  return 0;
}

int cfs_hip_sym_block_diagonal_async(cfs_hip_sym_t h, int block_rows, void *blocks_dev, void *stream) {
  if (!h || !blocks_dev) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (!block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "block diagonal: block_rows " + std::to_string(block_rows) + " is not one of 1, 2, 3, 4, 6");
  int rc = check_block_out(h, blocks_dev, "cfs_hip_sym_block_diagonal_async");
  if (rc) return rc;
  DeviceGuard g(h->device);
  return h->block_diagonal(blocks_dev, block_rows, (hipStream_t)stream);
}

int cfs_hip_sym_block_inverse_async(cfs_hip_sym_t h, int block_rows, void *minv_dev, void *stream) {
  if (!h || !minv_dev) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (!block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "block inverse: block_rows " + std::to_string(block_rows) + " is not one of 1, 2, 3, 4, 6");
  int rc = check_block_out(h, minv_dev, "cfs_hip_sym_block_inverse_async");
  if (rc) return rc;
  DeviceGuard g(h->device);
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    constexpr int BS = decltype(bs)::value;
    if constexpr (BS == 0) // (block_rows_ok: not reached)
      return set_err(CFS_HIP_ERR_INTERNAL, "block inverse: no blocks");
    else
      return cfs_solver::block_inverse<decltype(v), BS>(h, minv_dev, (hipStream_t)stream);
  });
}

int cfs_hip_sym_pcg_block(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int block_rows, double tol, int maxiter,
                          int check_every, int *iterations, double *relres, void *stream) {
  int rc = check_solve_args("pcg", "cg", "u and b", !h || !u_dev || !b_dev, u_dev, b_dev, &tol, maxiter, iterations, nullptr, relres);
  if (rc) return rc;
  if (!block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "pcg: block_rows " + std::to_string(block_rows) + " is not one of 1, 2, 3, 4, 6");
  if (block_rows == 1) // Jacobi: the same code path, the same bits
    return cfs_hip_sym_pcg(h, u_dev, b_dev, CFS_HIP_PRECOND_JACOBI, tol, maxiter, check_every, iterations, relres, stream);
  if ((rc = check_solve_handle(h, u_dev, b_dev, not_a_shard("pcg"), true, blocks_on_one_device("pcg", block_rows)))) return rc;
  return run_cg(h, u_dev, b_dev, block_rows, tol, maxiter, check_every, iterations, relres, stream);
}

int cfs_hip_sym_pcg_mixed(cfs_hip_sym_t h64, cfs_hip_sym_t h32, void *u_dev, const void *b_dev, int block_rows, double tol,
                          double delta, int maxiter, int check_every, int *iterations, int *replacements, double *relres,
                          void *stream) {
  int rc = check_solve_args("pcg_mixed", "pcg_mixed", "u and b", !h64 || !h32 || !u_dev || !b_dev, u_dev, b_dev, &tol, maxiter,
                            iterations, replacements, relres);
  if (rc) return rc;
  if (block_rows != 0 && !block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "pcg_mixed: block_rows " + std::to_string(block_rows) + " is not one of 0, 1, 2, 3, 4, 6");
  if (delta == 0.0) delta = 0.1;
  if (!(delta > 0.0 && delta < 1.0)) return set_err(CFS_HIP_ERR_ARG, "pcg_mixed: delta must lie in (0, 1) (0: the default, 0.1)");
  if (h64->value_bytes != 8 || h32->value_bytes != 4)
    return set_err(CFS_HIP_ERR_ARG, "pcg_mixed: the first handle must hold fp64 values and the second fp32 values (got " +
                                        std::to_string(h64->value_bytes) + " and " + std::to_string(h32->value_bytes) + " bytes)");
  if (h64->n() != h32->n())
    return set_err(CFS_HIP_ERR_ARG, "pcg_mixed: the handles hold matrices of " + std::to_string(h64->n()) + " and " +
                                        std::to_string(h32->n()) + " rows");
  for (cfs_hip_sym_t h : {h64, h32})
    if ((rc = check_whole_matrix(h, "pcg_mixed: handles of the whole matrix, not shards", true,
                                 "pcg_mixed: both matrices on one device (the multi-device form is not built)")))
      return rc;
  if (h64->device != h32->device)
    return set_err(CFS_HIP_ERR_ARG, "pcg_mixed: the fp64 matrix lives on device " + std::to_string(h64->device) +
                                        ", the fp32 matrix on device " + std::to_string(h32->device));
  if ((rc = check_placement(h64, u_dev, b_dev))) return rc;
  h64->ok_x = h64->ok_y = h32->ok_x = h32->ok_y = nullptr; // (as check_solve_handle, for both)
  DeviceGuard g(h64->device);
  return with_precond(4, block_rows, [&](auto, auto bs) {
    return cfs_solver::cg_mixed<decltype(bs)::value>(h64, h32, u_dev, b_dev, tol, delta, maxiter, check_every, iterations,
                                                     replacements, relres, (hipStream_t)stream);
  });
}

int cfs_hip_sym_minres(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int precond, double shift, double tol, int maxiter,
                       int check_every, int *iterations, double *relres, void *stream) {
  int rc = check_solve_args("minres", "minres", "u and b", !h || !u_dev || !b_dev, u_dev, b_dev, &tol, maxiter, iterations, nullptr, relres);
  if (rc) return rc;
  if (precond != CFS_HIP_PRECOND_NONE && precond != CFS_HIP_PRECOND_JACOBI)
    return set_err(CFS_HIP_ERR_ARG, "minres: unknown preconditioner " + std::to_string(precond));
  if (!std::isfinite(shift)) return set_err(CFS_HIP_ERR_ARG, "minres: the shift must be finite");
  if ((rc = check_solve_handle(h, u_dev, b_dev, not_a_shard("minres"), true, ""))) return rc;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return cfs_rt::with_value_type(h->value_bytes, [&](auto v) {
    typedef decltype(v) V;
    if (precond == CFS_HIP_PRECOND_JACOBI)
      return cfs_solver::minres<V, true>(h, u_dev, b_dev, shift, tol, maxiter, check_every, iterations, relres, st);
    return cfs_solver::minres<V, false>(h, u_dev, b_dev, shift, tol, maxiter, check_every, iterations, relres, st);
  });
}

// degree and the bounds of the Chebyshev entry points; need_both: both bounds must be given (> 0)
static int check_cheb_args(const char *who, int block_rows, int degree, double lmin, double lmax, bool need_both) {
  if (block_rows != 0 && !block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": block_rows " + std::to_string(block_rows) + " is not one of 0, 1, 2, 3, 4, 6");
  if (degree < 1 || degree > cfs_solver::kChebMaxDegree)
    return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": the degree must lie in [1, " + std::to_string(cfs_solver::kChebMaxDegree) +
                                        "], got " + std::to_string(degree));
  if (!std::isfinite(lmin) || !std::isfinite(lmax)) return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": the bounds must be finite");
  if (need_both && !(lmin > 0.0 && lmax > 0.0)) return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": both bounds must be given (> 0)");
  if (lmin > 0.0 && lmax > 0.0 && !(lmin < lmax))
    return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": lmin " + std::to_string(lmin) + " is not below lmax " + std::to_string(lmax));
  return 0;
}

int cfs_hip_sym_pcg_cheb(cfs_hip_sym_t h, void *u_dev, const void *b_dev, int block_rows, int degree, double lmin, double lmax,
                         double tol, int maxiter, int check_every, int *iterations, double *relres, double *bounds_used,
                         void *stream) {
  const char *who = "pcg_cheb";
  int rc = check_solve_args(who, who, "u and b", !h || !u_dev || !b_dev, u_dev, b_dev, &tol, maxiter, iterations, nullptr, relres);
  if (rc || (rc = check_cheb_args(who, block_rows, degree, lmin, lmax, false)) ||
      (rc = check_solve_handle(h, u_dev, b_dev, not_a_shard(who), true, blocks_on_one_device(who, block_rows))))
    return rc;
  DeviceGuard g(h->device);
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::cg_cheb<decltype(v), decltype(bs)::value>(h, u_dev, b_dev, degree, lmin, lmax, tol, maxiter, check_every,
                                                                 iterations, relres, bounds_used, (hipStream_t)stream);
  });
}

int cfs_hip_sym_cheb_apply(cfs_hip_sym_t h, int block_rows, int degree, double lmin, double lmax, void *z_dev, const void *r_dev,
                           void *stream) {
  const char *who = "cheb_apply";
  int rc = check_solve_args(who, who, "z and r", !h || !z_dev || !r_dev, z_dev, r_dev, nullptr, 0, nullptr, nullptr, nullptr);
  if (rc || (rc = check_cheb_args(who, block_rows, degree, lmin, lmax, true)) ||
      (rc = check_solve_handle(h, z_dev, r_dev, not_a_shard(who), true, blocks_on_one_device(who, block_rows))))
    return rc;
  DeviceGuard g(h->device);
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::cheb_apply<decltype(v), decltype(bs)::value>(h, degree, lmin, lmax, z_dev, r_dev, (hipStream_t)stream);
  });
}

int cfs_hip_sym_precond_lmax(cfs_hip_sym_t h, int block_rows, int steps, const void *v0_dev, double *estimate, void *stream) {
  if (!h || !estimate) return set_err(CFS_HIP_ERR_ARG, "null argument");
  *estimate = 0.0;
  if (block_rows != 0 && !block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "precond_lmax: block_rows " + std::to_string(block_rows) + " is not one of 0, 1, 2, 3, 4, 6");
  int rc = check_precond_handle(h, block_rows, "precond_lmax");
  if (rc) return rc;
  if (v0_dev) {
    const cfs_rt::PtrInfo pi = cfs_rt::classify(v0_dev);
    if (!pi.device) return set_err(CFS_HIP_ERR_ARG, "precond_lmax: v0 must be a device pointer");
    if (pi.dev != h->device)
      return set_err(CFS_HIP_ERR_ARG, "precond_lmax: v0 lives on device " + std::to_string(pi.dev) + ", the matrix on device " +
                                          std::to_string(h->device));
  }
  h->ok_x = h->ok_y = nullptr;
  DeviceGuard g(h->device);
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::cheb_lmax<decltype(v), decltype(bs)::value>(h, steps, v0_dev, estimate, (hipStream_t)stream);
  });
}

int cfs_hip_debug_cheb_coeffs(int degree, double lmin, double lmax, double *theta, double *c1, double *c2) {
  if (!theta || (degree > 1 && (!c1 || !c2))) return set_err(CFS_HIP_ERR_ARG, "null argument");
  int rc = check_cheb_args("cheb_coeffs", 0, degree, lmin, lmax, true);
  if (rc) return rc;
  cfs_solver::cheb_coeffs(degree, lmin, lmax, theta, c1, c2);
  return 0;
}

// ---- aggregation multigrid (cfs_solver_amg.hpp) ------------------------------------------------------
template <typename V>
static int amg_create(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const V *values, const cfs_hip_amg_options *opt,
                      cfs_hip_amg_t *out, bool refreshable = false, int matching = CFS_HIP_AMG_MATCHING_GREEDY, bool on_device = false,
                      int block = 1) {
  if (out) *out = nullptr;
  if (!h || !out || !rowptr || n < 0 || (n > 0 && rowptr[n] > 0 && (!colind || !values)))
    return set_err(CFS_HIP_ERR_ARG, "amg_create: null argument");
  const int passes = opt && opt->passes ? opt->passes : 2, degree = opt && opt->degree ? opt->degree : 1;
  const int coarse_max = opt && opt->coarse_max ? opt->coarse_max : 512;
  const double ratio = opt && opt->ratio != 0.0 ? opt->ratio : 4.0;
  if (passes < 1 || passes > 3) return set_err(CFS_HIP_ERR_ARG, "amg_create: passes must lie in [1, 3], got " + std::to_string(passes));
  if (degree < 1 || degree > 4) return set_err(CFS_HIP_ERR_ARG, "amg_create: the degree must lie in [1, 4], got " + std::to_string(degree));
  if (!std::isfinite(ratio) || !(ratio > 1.0))
    return set_err(CFS_HIP_ERR_ARG, "amg_create: the ratio lmax / lmin must be finite and > 1, got " + std::to_string(ratio));
  if (coarse_max < 1 || coarse_max > CFS_HIP_AMG_MAX_COARSE)
    return set_err(CFS_HIP_ERR_ARG, "amg_create: coarse_max must lie in [1, " + std::to_string(CFS_HIP_AMG_MAX_COARSE) + "], got " +
                                        std::to_string(coarse_max));
  SymMatrix<V> *m = dynamic_cast<SymMatrix<V> *>(h);
  if (!h->send_rows().empty() || h->rows() != h->n())
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "amg_create: a handle of the whole matrix, not a shard");
  int ngpus = 1;
  if (cfs_hip_sym_num_gpus(h, &ngpus) == 0 && ngpus != 1)
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "amg_create: the whole matrix on one device, not a multi-device handle");
  if (h->value_bytes != (int)sizeof(V) || !m)
    return set_err(CFS_HIP_ERR_ARG, "amg_create: the handle holds values of " + std::to_string(h->value_bytes) + " bytes, the CSR of " +
                                        std::to_string(sizeof(V)));
  if (n != h->n()) return set_err(CFS_HIP_ERR_ARG, "amg_create: n = " + std::to_string(n) + ", the handle has " + std::to_string(h->n()) + " rows");
  if (refreshable && m->P.deterministic)
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "amg_create_refreshable: a deterministic handle's levels are deterministic, and those refuse "
                                            "update_values (their fixed-point scale depends on the values)");
  if (on_device && n > 0 && 2 * (long long)rowptr[n] > (long long)INT_MAX)
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "amg_create_device: 2 nnz = " + std::to_string(2 * (long long)rowptr[n]) +
                                                " exceeds the 32-bit positions of the records");
  DeviceGuard g(h->device);
  const int flags = CFS_HIP_FLAG_NO_CALIBRATE | (m->P.deterministic ? CFS_HIP_FLAG_DETERMINISTIC : 0) |
                    (refreshable ? CFS_HIP_FLAG_KEEP_VALUE_MAP : 0);
  h->ok_x = h->ok_y = nullptr;
  auto make = [&](auto *obj) -> int { // obj: a new cfs_solver::Amg<V, BS>
    std::unique_ptr<std::remove_pointer_t<decltype(obj)>> a(obj);
    a->passes = passes, a->degree = degree, a->coarse_max = coarse_max, a->ratio = ratio, a->device = h->device;
    a->refreshable = refreshable, a->matching = matching, a->on_device = on_device ? 1 : 0;
    int rc = a->build(h, n, rowptr, colind, values, flags,
                      [](int ln, const int *rp, const int *ci, const V *va, int fl, cfs_hip_sym_s **lh) {
                        cfs_hip_options o = {0, 0, 0, fl};
                        return sym_create<V>(ln, rp, ci, va, 1, 0, nullptr, &o, lh);
                      });
    if (rc) return rc; // (the levels built so far go with `a`)
    *out = a.release();
    return 0;
  };
  switch (block) { // (cfs_hip_amg_create_block_* has checked it)
  case 2: return make(new cfs_solver::Amg<V, 2>());
  case 3: return make(new cfs_solver::Amg<V, 3>());
  case 4: return make(new cfs_solver::Amg<V, 4>());
  case 6: return make(new cfs_solver::Amg<V, 6>());
  default: return make(new cfs_solver::Amg<V, 1>());
  }
}
// block = 1: the scalar create with that matching itself
template <typename V>
static int amg_create_block(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const V *values, int block, int matching,
                            const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  if (out) *out = nullptr;
  if (block != 1 && block != 2 && block != 3 && block != 4 && block != 6)
    return set_err(CFS_HIP_ERR_ARG, "amg_create_block: block must be 1, 2, 3, 4 or 6, got " + std::to_string(block));
  if (matching != CFS_HIP_AMG_MATCHING_GREEDY && matching != CFS_HIP_AMG_MATCHING_DOMINANT)
    return set_err(CFS_HIP_ERR_ARG, "amg_create_block: matching must be CFS_HIP_AMG_MATCHING_GREEDY (0) or CFS_HIP_AMG_MATCHING_DOMINANT (1), got " +
                                        std::to_string(matching));
  if (n > 0 && n % block != 0)
    return set_err(CFS_HIP_ERR_ARG, "amg_create_block: n = " + std::to_string(n) + " is not a multiple of block = " + std::to_string(block) +
                                        " (a trailing partial node)");
  return amg_create<V>(h, n, rowptr, colind, values, opt, out, false, matching, false, block);
}
int cfs_hip_amg_create_block_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values, int block, int matching,
                                 const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create_block<double>(h, n, rowptr, colind, values, block, matching, opt, out);
}
int cfs_hip_amg_create_block_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values, int block, int matching,
                                 const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create_block<float>(h, n, rowptr, colind, values, block, matching, opt, out);
}
int cfs_hip_amg_block(cfs_hip_amg_t a, int *block) {
  if (!a || !block) return set_err(CFS_HIP_ERR_ARG, "amg_block: null argument");
  *block = a->block();
  return 0;
}
int cfs_hip_amg_level_node_weights(cfs_hip_amg_t a, int level, void *W) {
  if (!a || !W) return set_err(CFS_HIP_ERR_ARG, "amg_level_node_weights: null argument");
  return a->level_node_weights(level, W);
}
int cfs_hip_amg_create_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                           const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<double>(h, n, rowptr, colind, values, opt, out);
}
int cfs_hip_amg_create_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                           const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<float>(h, n, rowptr, colind, values, opt, out);
}
int cfs_hip_amg_create_refreshable_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                                       const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<double>(h, n, rowptr, colind, values, opt, out, true);
}
int cfs_hip_amg_create_refreshable_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                                       const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<float>(h, n, rowptr, colind, values, opt, out, true);
}
int cfs_hip_amg_create_dominant_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                                    const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<double>(h, n, rowptr, colind, values, opt, out, false, CFS_HIP_AMG_MATCHING_DOMINANT);
}
int cfs_hip_amg_create_dominant_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                                    const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<float>(h, n, rowptr, colind, values, opt, out, false, CFS_HIP_AMG_MATCHING_DOMINANT);
}
int cfs_hip_amg_create_device_f64(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const double *values,
                                  const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<double>(h, n, rowptr, colind, values, opt, out, false, CFS_HIP_AMG_MATCHING_DOMINANT, true);
}
int cfs_hip_amg_create_device_f32(cfs_hip_sym_t h, int n, const int *rowptr, const int *colind, const float *values,
                                  const cfs_hip_amg_options *opt, cfs_hip_amg_t *out) {
  return amg_create<float>(h, n, rowptr, colind, values, opt, out, false, CFS_HIP_AMG_MATCHING_DOMINANT, true);
}
int cfs_hip_amg_setup_info(cfs_hip_amg_t a, int *matching, int *on_device, int *rounds, double *seconds, long long *scratch_bytes) {
  if (!a) return set_err(CFS_HIP_ERR_ARG, "amg_setup_info: null argument");
  return a->setup_info(matching, on_device, rounds, seconds, scratch_bytes);
}
// cfs_hip_sym_update_values_* for a refreshable hierarchy: the same staging of a host array, the same stream
static int amg_update_values(cfs_hip_amg_t a, const void *values, long long nnz, size_t vb) {
  if (!a || !values) return set_err(CFS_HIP_ERR_ARG, "amg_update_values: null argument");
  if ((size_t)a->value_bytes != vb) return set_err(CFS_HIP_ERR_ARG, "amg_update_values: value type differs from the hierarchy's");
  int rc = a->update_check(nnz); // (not refreshable, another nnz: before any device work, and before a host array is read)
  if (rc) return rc;
  cfs_hip_sym_t h = a->fine;
  cfs_rt::DevCtx *ctx;
  if ((rc = cfs_rt::device_ctx(h->device, &ctx))) return rc;
  DeviceGuard g(h->device);
  const cfs_rt::PtrInfo vi = cfs_rt::classify(values);
  if (vi.device && vi.dev != h->device) return set_err(CFS_HIP_ERR_ARG, "amg_update_values: values live on another device than the matrix");
  DevBuf tmp;
  const void *src = values;
  if (!vi.device) {
    if ((rc = tmp.alloc((size_t)nnz * vb))) return rc;
    HIPCHK(hipMemcpyAsync(tmp.p, values, (size_t)nnz * vb, hipMemcpyHostToDevice, ctx->stream));
    src = tmp.p;
  }
  h->ok_x = h->ok_y = nullptr;
  rc = a->update_values(src, nnz, ctx->stream);
  HIPCHK(hipStreamSynchronize(ctx->stream)); // tmp goes away; a cycle enqueued afterwards on any stream sees the hierarchy
  return rc;
}
int cfs_hip_amg_update_values_f64(cfs_hip_amg_t a, const double *values, long long nnz) { return amg_update_values(a, values, nnz, 8); }
int cfs_hip_amg_update_values_f32(cfs_hip_amg_t a, const float *values, long long nnz) { return amg_update_values(a, values, nnz, 4); }
int cfs_hip_amg_refresh_info(cfs_hip_amg_t a, long long *map_bytes, int *refreshes, double *last_seconds) {
  if (!a) return set_err(CFS_HIP_ERR_ARG, "amg_refresh_info: null argument");
  return a->refresh_info(map_bytes, refreshes, last_seconds, nullptr);
}
int cfs_hip_debug_amg_refresh_split(cfs_hip_amg_t a, double *seconds) {
  if (!a || !seconds) return set_err(CFS_HIP_ERR_ARG, "amg_refresh_split: null argument");
  return a->refresh_info(nullptr, nullptr, nullptr, seconds);
}
int cfs_hip_debug_amg_recoarsen(int n, const int *rowptr, const int *colind, const double *values_at_create, const double *values_new,
                                int passes, double *w, double *c_values, long long capacity, long long *c_nnz) {
  if (n < 0 || !rowptr || !w || !c_nnz || (n > 0 && rowptr[n] > 0 && (!colind || !values_at_create || !values_new)))
    return set_err(CFS_HIP_ERR_ARG, "amg_recoarsen: null argument");
  if (passes < 1 || passes > 3) return set_err(CFS_HIP_ERR_ARG, "amg_recoarsen: passes must lie in [1, 3], got " + std::to_string(passes));
  cfs_solver::AmgCsr low, coarse;
  cfs_solver::amg_lower(n, rowptr, colind, values_at_create, low);
  cfs_solver::AmgList lists;
  cfs_solver::amg_lower_lists(n, rowptr, colind, lists);
  cfs_solver::AmgFrozen frozen;
  std::vector<int> ag;
  std::vector<double> wv, a_new((size_t)low.nnz()), out;
  long long bad = 0;
  if (cfs_solver::amg_coarsen(low, passes, ag, wv, coarse, &bad, &frozen))
    return set_err(CFS_HIP_ERR_ARG, "amg_recoarsen: Jacobi needs a positive diagonal, " + std::to_string(bad) + " of " + std::to_string(n) +
                                        " entries (at create) are zero, negative or not finite");
  if (frozen.overflow()) return set_err(CFS_HIP_ERR_UNSUPPORTED, "amg_recoarsen: the contributions of a round exceed the 32-bit indices of the lists");
  cfs_solver::amg_eval_list(lists, values_new, a_new.data());
  for (int i = 0; i < n; ++i) {
    const double d = a_new[frozen.diag[i]];
    if (!(d > 0.0) || d * 0.0 != 0.0) bad += 1;
  }
  if (bad)
    return set_err(CFS_HIP_ERR_ARG, "amg_recoarsen: Jacobi needs a positive diagonal, " + std::to_string(bad) + " of " + std::to_string(n) +
                                        " entries are zero, negative or not finite");
  cfs_solver::amg_eval_frozen(frozen, low.ci, a_new.data(), wv, out);
  *c_nnz = (long long)out.size();
  for (int i = 0; i < n; ++i) w[i] = wv[i];
  if ((long long)out.size() > capacity || (!out.empty() && !c_values))
    return set_err(CFS_HIP_ERR_ARG, "amg_recoarsen: the coarse matrix has " + std::to_string(out.size()) + " entries, room for " +
                                        std::to_string(capacity));
  for (size_t k = 0; k < out.size(); ++k) c_values[k] = out[k];
  return 0;
}
int cfs_hip_amg_destroy(cfs_hip_amg_t a) {
  delete a;
  return 0;
}
int cfs_hip_amg_info(cfs_hip_amg_t a, cfs_hip_amg_info_t *out) {
  if (!a || !out) return set_err(CFS_HIP_ERR_ARG, "amg_info: null argument");
  return a->info(out);
}
int cfs_hip_amg_level_aggregates(cfs_hip_amg_t a, int level, int *agg, void *w) {
  if (!a) return set_err(CFS_HIP_ERR_ARG, "amg_level_aggregates: null argument");
  return a->level_aggregates(level, agg, w);
}
int cfs_hip_amg_level_matrix(cfs_hip_amg_t a, int level, int *rowptr, int *colind, void *values) {
  if (!a) return set_err(CFS_HIP_ERR_ARG, "amg_level_matrix: null argument");
  return a->level_matrix(level, rowptr, colind, values);
}
int cfs_hip_amg_coarse_inverse(cfs_hip_amg_t a, void *inv) {
  if (!a || !inv) return set_err(CFS_HIP_ERR_ARG, "amg_coarse_inverse: null argument");
  return a->coarse_inverse(inv);
}
int cfs_hip_amg_apply(cfs_hip_amg_t a, void *z_dev, const void *r_dev, void *stream) {
  const char *who = "amg_apply";
  int rc = check_solve_args(who, who, "z and r", !a || !z_dev || !r_dev, z_dev, r_dev, nullptr, 0, nullptr, nullptr, nullptr,
                            "amg_apply: null argument");
  cfs_hip_sym_t h = rc ? nullptr : a->fine; // (a handle cfs_hip_amg_create_* accepted: the whole matrix on one device)
  if (rc || (rc = check_solve_handle(h, z_dev, r_dev, not_a_shard(who), true, ""))) return rc;
  DeviceGuard g(h->device);
  return a->apply(z_dev, r_dev, (hipStream_t)stream);
}
int cfs_hip_amg_apply_cols(cfs_hip_amg_t a, void *z_dev, const void *r_dev, long long ld, int ncols, unsigned active, void *stream) {
  const char *who = "amg_apply_cols";
  if (!a || !z_dev || !r_dev) return set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: null argument");
  if (ncols < 1 || ncols > CFS_HIP_LOBPCG_MAX_K)
    return set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: 1 <= ncols <= " + std::to_string(CFS_HIP_LOBPCG_MAX_K) + ", got " + std::to_string(ncols));
  if (active >> ncols) return set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: active names a column that is not in [0, ncols)");
  if ((((uintptr_t)z_dev) | ((uintptr_t)r_dev)) & 15) return set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: Z and R must be 16-byte aligned");
  cfs_hip_sym_t h = a->fine;
  const long long n = h->n(), vb = a->value_bytes;
  if (ld < n || ld > (1LL << 56) || (ncols > 1 && (ld * vb) % 16 != 0))
    return set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: bad ld " + std::to_string(ld) + ": at least n = " + std::to_string(n) +
                                        " and, for more than one column, a multiple of 16 bytes");
  const uintptr_t span = (uintptr_t)(((long long)(ncols - 1) * ld + n) * vb), z0 = (uintptr_t)z_dev, r0 = (uintptr_t)r_dev;
  if (z0 < r0 + span && r0 < z0 + span) return set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: the blocks Z and R overlap");
  if (a->is_stale()) return set_err(CFS_HIP_ERR_ARG, "amg_apply_cols: the last refresh failed");
  int rc = check_solve_handle(h, z_dev, r_dev, not_a_shard(who), true, "");
  if (rc) return rc;
  if (active == 0) return 0;
  DeviceGuard g(h->device);
  return a->apply_cols(z_dev, r_dev, ld, ncols, active, (hipStream_t)stream);
}
int cfs_hip_amg_column_cycles(cfs_hip_amg_t a, long long *cycles) {
  if (!a || !cycles) return set_err(CFS_HIP_ERR_ARG, "amg_column_cycles: null argument");
  *cycles = a->column_cycles();
  return 0;
}
int cfs_hip_sym_pcg_amg(cfs_hip_sym_t h, cfs_hip_amg_t a, void *u_dev, const void *b_dev, double tol, int maxiter, int check_every,
                        int *iterations, double *relres, void *stream) {
  (void)check_every; // (the host looks after every iteration: cfs_hip.h)
  const char *who = "pcg_amg";
  int rc = check_solve_args(who, who, "u and b", !h || !a || !u_dev || !b_dev, u_dev, b_dev, &tol, maxiter, iterations, nullptr, relres);
  if (rc || (rc = check_whole_matrix(h, not_a_shard(who), true, "pcg_amg: the whole matrix on one device, not a multi-device handle")))
    return rc;
  if (a->fine != h) return set_err(CFS_HIP_ERR_ARG, "pcg_amg: the hierarchy was created on another handle");
  if ((rc = check_placement(h, u_dev, b_dev))) return rc;
  h->ok_x = h->ok_y = nullptr; // (as check_solve_handle)
  DeviceGuard g(h->device);
  return a->pcg(u_dev, b_dev, tol, maxiter, iterations, relres, (hipStream_t)stream);
}
// ---- PCG on a block of right-hand sides -------------------------------------------------------------
// What cfs_hip_sym_pcg_cols and cfs_hip_sym_pcg_amg_cols check of their blocks before they look at the handle's
// placement, in the order cfs_hip.h documents: null, ncols, alignment, ld, overlap, tol / maxiter.  The outputs are
// zeroed as soon as their length is known to be sane.
static int check_cols_args(const char *who, bool any_null, cfs_hip_sym_t h, const void *u, const void *b, long long ld, int ncols,
                           double tol, int maxiter, int *iterations, double *relres) {
  const std::string w(who);
  if (any_null) return set_err(CFS_HIP_ERR_ARG, w + ": null argument");
  if (iterations) iterations[0] = 0;
  if (relres) relres[0] = 0.0;
  if (ncols < 1 || ncols > CFS_HIP_LOBPCG_MAX_K)
    return set_err(CFS_HIP_ERR_ARG, w + ": 1 <= ncols <= " + std::to_string(CFS_HIP_LOBPCG_MAX_K) + ", got " + std::to_string(ncols));
  for (int c = 0; c < ncols; ++c) {
    if (iterations) iterations[c] = 0;
    if (relres) relres[c] = 0.0;
  }
  if ((((uintptr_t)u) | ((uintptr_t)b)) & 15) return set_err(CFS_HIP_ERR_ARG, w + ": U and B must be 16-byte aligned");
  const long long n = h->n(), vb = h->value_bytes;
  if (ld < n || ld > (1LL << 56) || (ncols > 1 && (ld * vb) % 16 != 0))
    return set_err(CFS_HIP_ERR_ARG, w + ": bad ld " + std::to_string(ld) + ": at least n = " + std::to_string(n) +
                                        " and, for more than one column, a multiple of 16 bytes");
  const uintptr_t span = (uintptr_t)(((long long)(ncols - 1) * ld + n) * vb), u0 = (uintptr_t)u, b0 = (uintptr_t)b;
  if (u0 < b0 + span && b0 < u0 + span) return set_err(CFS_HIP_ERR_ARG, w + ": the blocks U and B overlap");
  if (maxiter < 0 || !(tol >= 0.0)) return set_err(CFS_HIP_ERR_ARG, w + ": bad tolerance / iteration limit");
  return 0;
}

int cfs_hip_sym_pcg_cols(cfs_hip_sym_t h, void *u_dev, const void *b_dev, long long ld, int ncols, int block_rows, double tol,
                         int maxiter, int check_every, int *iterations, double *relres, void *stream) {
  const char *who = "pcg_cols";
  int rc = check_cols_args(who, !h || !u_dev || !b_dev, h, u_dev, b_dev, ld, ncols, tol, maxiter, iterations, relres);
  if (rc) return rc;
  if (block_rows != 0 && !block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "pcg_cols: block_rows " + std::to_string(block_rows) + " is not one of 0, 1, 2, 3, 4, 6");
  if ((rc = check_whole_matrix(h, not_a_shard(who), true, "pcg_cols: the whole matrix on one device, not a multi-device handle")) ||
      (rc = check_placement(h, u_dev, b_dev)))
    return rc;
  h->ok_x = h->ok_y = nullptr; // (as check_solve_handle)
  DeviceGuard g(h->device);
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::cg_cols<decltype(v), decltype(bs)::value>(h, u_dev, b_dev, ld, ncols, tol, maxiter, check_every, iterations, relres,
                                                                 (hipStream_t)stream);
  });
}

int cfs_hip_sym_pcg_amg_cols(cfs_hip_sym_t h, cfs_hip_amg_t a, void *u_dev, const void *b_dev, long long ld, int ncols, double tol,
                             int maxiter, int check_every, int *iterations, double *relres, void *stream) {
  (void)check_every; // (the host looks after every iteration, as in cfs_hip_sym_pcg_amg)
  const char *who = "pcg_amg_cols";
  int rc = check_cols_args(who, !h || !a || !u_dev || !b_dev, h, u_dev, b_dev, ld, ncols, tol, maxiter, iterations, relres);
  if (rc || (rc = check_whole_matrix(h, not_a_shard(who), true, "pcg_amg_cols: the whole matrix on one device, not a multi-device handle")))
    return rc;
  if (a->fine != h) return set_err(CFS_HIP_ERR_ARG, "pcg_amg_cols: the hierarchy was created on another handle");
  if (a->is_stale()) return set_err(CFS_HIP_ERR_ARG, "pcg_amg_cols: the last refresh failed");
  if ((rc = check_placement(h, u_dev, b_dev))) return rc;
  h->ok_x = h->ok_y = nullptr; // (as check_solve_handle)
  DeviceGuard g(h->device);
  return a->pcg_cols(u_dev, b_dev, ld, ncols, tol, maxiter, iterations, relres, (hipStream_t)stream);
}
static int amg_coarsen_entry(int n, const int *rowptr, const int *colind, const double *values, int passes, int *agg, double *w, int *nc,
                             int *c_rowptr, int *c_colind, double *c_values, long long capacity, long long *c_nnz, int matching, int *rounds) {
  if (n < 0 || !rowptr || !agg || !w || !nc || !c_rowptr || !c_nnz || (n > 0 && rowptr[n] > 0 && (!colind || !values)) ||
      (matching == CFS_HIP_AMG_MATCHING_DOMINANT && !rounds))
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen: null argument");
  if (passes < 1 || passes > 3) return set_err(CFS_HIP_ERR_ARG, "amg_coarsen: passes must lie in [1, 3], got " + std::to_string(passes));
  cfs_solver::AmgCsr low, coarse;
  cfs_solver::amg_lower(n, rowptr, colind, values, low);
  std::vector<int> ag;
  std::vector<double> wv;
  long long bad = 0;
  if (cfs_solver::amg_coarsen(low, passes, ag, wv, coarse, &bad, nullptr, matching, rounds))
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen: Jacobi needs a positive diagonal, " + std::to_string(bad) + " of " + std::to_string(n) +
                                        " entries are zero, negative or not finite");
  *nc = coarse.n;
  *c_nnz = coarse.nnz();
  for (int i = 0; i < n; ++i) agg[i] = ag[i], w[i] = wv[i];
  for (int i = 0; i <= coarse.n; ++i) c_rowptr[i] = (int)coarse.rp[i];
  if (coarse.nnz() > capacity || (coarse.nnz() > 0 && (!c_colind || !c_values)))
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen: the coarse matrix has " + std::to_string(coarse.nnz()) + " entries, room for " +
                                        std::to_string(capacity));
  for (long long k = 0; k < coarse.nnz(); ++k) c_colind[k] = coarse.ci[k], c_values[k] = coarse.va[k];
  return 0;
}
int cfs_hip_debug_amg_coarsen(int n, const int *rowptr, const int *colind, const double *values, int passes, int *agg, double *w,
                              int *nc, int *c_rowptr, int *c_colind, double *c_values, long long capacity, long long *c_nnz) {
  return amg_coarsen_entry(n, rowptr, colind, values, passes, agg, w, nc, c_rowptr, c_colind, c_values, capacity, c_nnz,
                           CFS_HIP_AMG_MATCHING_GREEDY, nullptr);
}
int cfs_hip_debug_amg_coarsen_dominant(int n, const int *rowptr, const int *colind, const double *values, int passes, int *agg, double *w,
                                       int *nc, int *c_rowptr, int *c_colind, double *c_values, long long capacity, long long *c_nnz,
                                       int *rounds) {
  return amg_coarsen_entry(n, rowptr, colind, values, passes, agg, w, nc, c_rowptr, c_colind, c_values, capacity, c_nnz,
                           CFS_HIP_AMG_MATCHING_DOMINANT, rounds);
}
int cfs_hip_debug_amg_coarsen_block(int n, const int *rowptr, const int *colind, const double *values, int block, int passes, int matching,
                                    int *agg, double *W, int *nc, int *c_rowptr, int *c_colind, double *c_values, long long capacity,
                                    long long *c_nnz, int *rounds) {
  if (block != 1 && block != 2 && block != 3 && block != 4 && block != 6)
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen_block: block must be 1, 2, 3, 4 or 6, got " + std::to_string(block));
  if (matching != CFS_HIP_AMG_MATCHING_GREEDY && matching != CFS_HIP_AMG_MATCHING_DOMINANT)
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen_block: matching must be CFS_HIP_AMG_MATCHING_GREEDY (0) or CFS_HIP_AMG_MATCHING_DOMINANT (1), got " +
                                        std::to_string(matching));
  int own_rounds[3] = {0, 0, 0};
  if (!rounds) rounds = own_rounds;
  if (block == 1)
    return amg_coarsen_entry(n, rowptr, colind, values, passes, agg, W, nc, c_rowptr, c_colind, c_values, capacity, c_nnz, matching,
                             matching == CFS_HIP_AMG_MATCHING_DOMINANT ? rounds : nullptr);
  if (n < 0 || !rowptr || !agg || !W || !nc || !c_rowptr || !c_nnz || (n > 0 && rowptr[n] > 0 && (!colind || !values)))
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen_block: null argument");
  if (passes < 1 || passes > 3) return set_err(CFS_HIP_ERR_ARG, "amg_coarsen_block: passes must lie in [1, 3], got " + std::to_string(passes));
  if (n % block != 0)
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen_block: n = " + std::to_string(n) + " is not a multiple of block = " + std::to_string(block) +
                                        " (a trailing partial node)");
  cfs_solver::AmgCsr low, coarse;
  cfs_solver::amg_lower(n, rowptr, colind, values, low);
  std::vector<int> ag;
  std::vector<double> wv;
  long long bad = 0;
  if (cfs_solver::amg_coarsen_block(low, block, passes, ag, wv, coarse, &bad, matching, rounds))
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen_block: node-block multigrid needs positive definite node blocks, " + std::to_string(bad) +
                                        " of " + std::to_string(n / block) + " blocks of " + std::to_string(block) +
                                        " rows have an eigenvalue that is zero, negative or not finite (level 0)");
  *nc = coarse.n;
  *c_nnz = coarse.nnz();
  for (int i = 0; i < n; ++i) agg[i] = ag[i];
  for (size_t k = 0; k < wv.size(); ++k) W[k] = wv[k];
  for (int i = 0; i <= coarse.n; ++i) c_rowptr[i] = (int)coarse.rp[i];
  if (coarse.nnz() > capacity || (coarse.nnz() > 0 && (!c_colind || !c_values)))
    return set_err(CFS_HIP_ERR_ARG, "amg_coarsen_block: the coarse matrix has " + std::to_string(coarse.nnz()) + " entries, room for " +
                                        std::to_string(capacity));
  for (long long k = 0; k < coarse.nnz(); ++k) c_colind[k] = coarse.ci[k], c_values[k] = coarse.va[k];
  return 0;
}

// a vector argument of the eigensolver entry points: device memory on the handle's device
static int check_eigs_ptr(cfs_hip_sym_t h, const void *p, const char *who, const char *what) {
  const cfs_rt::PtrInfo pi = cfs_rt::classify(p);
  if (!pi.device) return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": " + what + " must be a device pointer");
  if (pi.dev != h->device)
    return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": " + what + " lives on device " + std::to_string(pi.dev) +
                                        ", the matrix on device " + std::to_string(h->device));
  return 0;
}

int cfs_hip_sym_eigs(cfs_hip_sym_t h, int k, int which, int ncv, double tol, int max_restarts, const void *v0_dev,
                     double *eigenvalues, void *vectors_dev, long long ld, double *residuals, int *nconv, int *restarts,
                     int *products, void *stream) {
  if (!h || !eigenvalues) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (nconv) *nconv = 0;
  if (restarts) *restarts = 0;
  if (products) *products = 0;
  if (which != CFS_HIP_EIGS_LARGEST && which != CFS_HIP_EIGS_SMALLEST && which != CFS_HIP_EIGS_MAGNITUDE)
    return set_err(CFS_HIP_ERR_ARG, "eigs: unknown which " + std::to_string(which));
  if (k < 1 || ncv < 0 || ncv > CFS_HIP_EIGS_MAX_NCV || (ncv != 0 && k >= ncv) || k >= CFS_HIP_EIGS_MAX_NCV)
    return set_err(CFS_HIP_ERR_ARG, "eigs: bad k / ncv: 1 <= k < ncv <= min(n, " + std::to_string(CFS_HIP_EIGS_MAX_NCV) +
                                        ") (ncv = 0: the default), got k = " + std::to_string(k) + ", ncv = " + std::to_string(ncv));
  if (!(tol >= 0.0) || max_restarts < 0) return set_err(CFS_HIP_ERR_ARG, "eigs: bad tolerance / restart limit");
  if ((((uintptr_t)v0_dev) | ((uintptr_t)vectors_dev)) & 15)
    return set_err(CFS_HIP_ERR_ARG, "eigs: v0 and the vectors must be 16-byte aligned");
  if (!h->send_rows().empty() || h->rows() != h->n())
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "eigs: a handle of the whole matrix, not a shard");
  const long long n = h->n();
  if (ncv == 0) ncv = (int)std::min<long long>(n, std::max(2 * k + 1, 20));
  if (ncv > n || k >= ncv)
    return set_err(CFS_HIP_ERR_ARG, "eigs: bad k / ncv: 1 <= k < ncv <= min(n, " + std::to_string(CFS_HIP_EIGS_MAX_NCV) +
                                        "), got k = " + std::to_string(k) + ", ncv = " + std::to_string(ncv) + ", n = " + std::to_string(n));
  if (vectors_dev && (ld < n || (ld * h->value_bytes) % 16 != 0))
    return set_err(CFS_HIP_ERR_ARG, "eigs: bad ld " + std::to_string(ld) + ": at least n = " + std::to_string(n) +
                                        " and a multiple of 16 bytes");
  int rc;
  if (v0_dev && (rc = check_eigs_ptr(h, v0_dev, "eigs", "v0"))) return rc;
  if (vectors_dev && (rc = check_eigs_ptr(h, vectors_dev, "eigs", "the vectors"))) return rc;
  h->ok_x = h->ok_y = nullptr; // (the iteration's own vectors are library memory on the handle's device)
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return cfs_rt::with_value_type(h->value_bytes, [&](auto v) {
    return cfs_solver::eigs<decltype(v)>(h, k, which, ncv, tol, max_restarts, v0_dev, eigenvalues, vectors_dev, ld, residuals, nconv,
                                         restarts, products, st);
  });
}

int cfs_hip_sym_debug_lanczos(cfs_hip_sym_t h, const void *v0_dev, int steps, void *basis_dev, long long ld, double *alpha,
                              double *beta, int *done, void *stream) {
  if (!h || !basis_dev || !alpha || !beta || !done) return set_err(CFS_HIP_ERR_ARG, "null argument");
  *done = 0;
  if (steps < 1 || steps > CFS_HIP_EIGS_MAX_NCV)
    return set_err(CFS_HIP_ERR_ARG, "lanczos: steps must lie in [1, " + std::to_string(CFS_HIP_EIGS_MAX_NCV) + "]");
  if ((((uintptr_t)v0_dev) | ((uintptr_t)basis_dev)) & 15)
    return set_err(CFS_HIP_ERR_ARG, "lanczos: v0 and the basis must be 16-byte aligned");
  if (!h->send_rows().empty() || h->rows() != h->n())
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "lanczos: a handle of the whole matrix, not a shard");
  if (ld < h->n() || (ld * h->value_bytes) % 16 != 0)
    return set_err(CFS_HIP_ERR_ARG, "lanczos: bad ld " + std::to_string(ld) + ": at least n and a multiple of 16 bytes");
  int rc;
  if (v0_dev && (rc = check_eigs_ptr(h, v0_dev, "lanczos", "v0"))) return rc;
  if ((rc = check_eigs_ptr(h, basis_dev, "lanczos", "the basis"))) return rc;
  h->ok_x = h->ok_y = nullptr;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return cfs_rt::with_value_type(h->value_bytes, [&](auto v) {
    return cfs_solver::debug_lanczos<decltype(v)>(h, v0_dev, steps, basis_dev, ld, alpha, beta, done, st);
  });
}

int cfs_hip_debug_symeig(int m, const double *a, double *w, double *s) {
  if (!a || !w || !s) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (m < 1 || m > CFS_HIP_EIGS_MAX_NCV)
    return set_err(CFS_HIP_ERR_ARG, "symeig: m must lie in [1, " + std::to_string(CFS_HIP_EIGS_MAX_NCV) + "]");
  if (cfs_solver::symeig(m, a, w, s) < 0) return set_err(CFS_HIP_ERR_INTERNAL, "symeig: no convergence");
  return 0;
}

int cfs_hip_debug_eigs_combine(void *out_dev, long long ldo, const void *basis_dev, long long ld, long long n, int m, int nout,
                               const double *s, int value_bytes, void *stream) {
  if (!out_dev || !basis_dev || !s) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (m < 1 || m > CFS_HIP_EIGS_MAX_NCV || nout < 1 || nout > m)
    return set_err(CFS_HIP_ERR_ARG, "eigs_combine: bad m / nout: 1 <= nout <= m <= " + std::to_string(CFS_HIP_EIGS_MAX_NCV) + ", got m = " +
                                        std::to_string(m) + ", nout = " + std::to_string(nout));
  if (value_bytes != 4 && value_bytes != 8) return set_err(CFS_HIP_ERR_ARG, "eigs_combine: value_bytes must be 4 or 8");
  if ((((uintptr_t)out_dev) | ((uintptr_t)basis_dev)) & 15)
    return set_err(CFS_HIP_ERR_ARG, "eigs_combine: out and the basis must be 16-byte aligned");
  // (the upper limit keeps the byte spans below within 63 bits)
  const long long ldmax = (1LL << 62) / (8LL * CFS_HIP_EIGS_MAX_NCV);
  if (n < 1 || ld < n || ldo < n || ld > ldmax || ldo > ldmax || (ld * value_bytes) % 16 != 0 || (ldo * value_bytes) % 16 != 0)
    return set_err(CFS_HIP_ERR_ARG, "eigs_combine: bad ld " + std::to_string(ld) + " / ldo " + std::to_string(ldo) + ": at least n = " +
                                        std::to_string(n) + " >= 1 and a multiple of 16 bytes");
  // the two blocks, first byte to the last row of the last column: the same block (the in-place restart), or disjoint
  const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)(((long long)(nout - 1) * ldo + n) * value_bytes);
  const uintptr_t b0 = (uintptr_t)basis_dev, b1 = b0 + (uintptr_t)(((long long)(m - 1) * ld + n) * value_bytes);
  if (!(o0 == b0 && ldo == ld) && o0 < b1 && b0 < o1)
    return set_err(CFS_HIP_ERR_ARG, "eigs_combine: out and the basis overlap: the same block with ldo == ld (in place), or disjoint");
  int cur = -1;
  HIPCHK(hipGetDevice(&cur));
  for (const void *p : {(const void *)out_dev, basis_dev}) {
    const cfs_rt::PtrInfo pi = cfs_rt::classify(p);
    if (!pi.device || pi.dev != cur) return set_err(CFS_HIP_ERR_ARG, "eigs_combine: out and the basis must be device memory of the current device");
  }
  return cfs_rt::with_value_type(value_bytes, [&](auto v) {
    return cfs_solver::debug_eigs_combine<decltype(v)>(out_dev, ldo, basis_dev, ld, n, m, nout, s, (hipStream_t)stream);
  });
}

// ---- LOBPCG ----
// the checks that cfs_hip_sym_lobpcg and cfs_hip_sym_debug_lobpcg share, from "bad k" on, in the documented order
// (a: the hierarchy of the multigrid form, whose value type must be the handle's -- asked when the handle is first read)
static int check_lobpcg(cfs_hip_sym_t h, int k, int block_rows, bool tol_ok, const void *x0_dev, long long ld0, const void *vectors_dev,
                        long long ld, cfs_hip_amg_t a = nullptr, cfs_hip_sym_t hb = nullptr) {
  if (k < 1 || k > CFS_HIP_LOBPCG_MAX_K)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg: bad k: 1 <= k <= " + std::to_string(CFS_HIP_LOBPCG_MAX_K) + " and 3 k <= n, got k = " + std::to_string(k));
  if (block_rows != 0 && !block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "lobpcg: block_rows " + std::to_string(block_rows) + " is not one of 0, 1, 2, 3, 4, 6");
  if (!tol_ok) return set_err(CFS_HIP_ERR_ARG, "lobpcg: bad tolerance / scale / iteration limit");
  if ((((uintptr_t)x0_dev) | ((uintptr_t)vectors_dev)) & 15)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg: x0 and the vectors must be 16-byte aligned");
  if (a && a->value_bytes != h->value_bytes) return set_err(CFS_HIP_ERR_ARG, "lobpcg_amg: value type differs from the hierarchy's");
  // (hb: the B of the pencil forms -- h's n, value type and device; then no shard and one device on either side)
  if (hb && (hb->n() != h->n() || hb->value_bytes != h->value_bytes || hb->device != h->device))
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_gen: B must have the n, the value type and the device of A: n " + std::to_string(hb->n()) +
                                        " / " + std::to_string(h->n()) + ", value bytes " + std::to_string(hb->value_bytes) + " / " +
                                        std::to_string(h->value_bytes) + ", device " + std::to_string(hb->device) + " / " +
                                        std::to_string(h->device));
  if (!h->send_rows().empty() || h->rows() != h->n())
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "lobpcg: a handle of the whole matrix, not a shard");
  if (hb) {
    int rc2;
    const std::string one = "lobpcg_gen: the whole matrix on one device, not a multi-device handle";
    if ((rc2 = check_whole_matrix(hb, not_a_shard("lobpcg_gen: B"), true, "")) || (rc2 = check_whole_matrix(h, not_a_shard("lobpcg_gen"), true, one)) ||
        (rc2 = check_whole_matrix(hb, not_a_shard("lobpcg_gen: B"), true, one)))
      return rc2;
  }
  const long long n = h->n();
  if (3LL * k > n)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg: bad k: 1 <= k <= " + std::to_string(CFS_HIP_LOBPCG_MAX_K) + " and 3 k <= n, got k = " + std::to_string(k) +
                                        ", n = " + std::to_string(n));
  if (ld < n || (ld * h->value_bytes) % 16 != 0 || (x0_dev && (ld0 < n || (ld0 * h->value_bytes) % 16 != 0)))
    return set_err(CFS_HIP_ERR_ARG, "lobpcg: bad ld " + std::to_string(ld) + " / ld0 " + std::to_string(ld0) + ": at least n = " +
                                        std::to_string(n) + " and a multiple of 16 bytes");
  if (block_rows >= 2) {
    int ngpus = 1;
    if (cfs_hip_sym_num_gpus(h, &ngpus) == 0 && ngpus != 1)
      return set_err(CFS_HIP_ERR_UNSUPPORTED, "lobpcg: block Jacobi needs the whole matrix on one device (blocks straddle the "
                                              "row splits of a multi-device handle)");
  }
  int rc;
  if (x0_dev && (rc = check_eigs_ptr(h, x0_dev, "lobpcg", "x0"))) return rc;
  return check_eigs_ptr(h, vectors_dev, "lobpcg", "the vectors");
}

int cfs_hip_sym_lobpcg(cfs_hip_sym_t h, int k, int block_rows, double tol, double scale, int maxiter, const void *x0_dev,
                       long long ld0, double *eigenvalues, void *vectors_dev, long long ld, double *residuals, int *nconv,
                       int *iterations, int *products, void *stream) {
  if (!h || !eigenvalues || !vectors_dev) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (nconv) *nconv = 0;
  if (iterations) *iterations = 0;
  if (products) *products = 0;
  const bool tol_ok = tol >= 0.0 && scale > 0.0 && std::isfinite(scale) && maxiter >= 0;
  int rc = check_lobpcg(h, k, block_rows, tol_ok, x0_dev, ld0, vectors_dev, ld);
  if (rc) return rc;
  h->ok_x = h->ok_y = nullptr; // (the iteration's own vectors are library memory on the handle's device)
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::lobpcg<decltype(v), decltype(bs)::value, false>(h, (cfs_hip_sym_t) nullptr, k, tol, scale, maxiter, -1, x0_dev, ld0,
                                                                       eigenvalues, vectors_dev, ld, residuals, nconv, iterations, products,
                                                                       nullptr, st);
  });
}

int cfs_hip_sym_debug_lobpcg(cfs_hip_sym_t h, int k, int block_rows, const void *x0_dev, long long ld0, int iters, double *theta,
                             void *vectors_dev, long long ld, double *resnorms, void *stream) {
  if (!h || !theta || !vectors_dev || !resnorms) return set_err(CFS_HIP_ERR_ARG, "null argument");
  int rc = check_lobpcg(h, k, block_rows, iters >= 0, x0_dev, ld0, vectors_dev, ld);
  if (rc) return rc;
  h->ok_x = h->ok_y = nullptr;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::lobpcg<decltype(v), decltype(bs)::value, false>(h, (cfs_hip_sym_t) nullptr, k, 0.0, 1.0, 0, iters, x0_dev, ld0, theta,
                                                                       vectors_dev, ld, resnorms, nullptr, nullptr, nullptr, nullptr, st);
  });
}

// the checks of the two multigrid forms behind their null checks: check_lobpcg (no stored M^-1: block_rows 0; the
// hierarchy's value type), one device as cfs_hip_sym_pcg_amg asks, the hierarchy created on h and not stale
static int check_lobpcg_amg(cfs_hip_sym_t h, cfs_hip_amg_t a, int k, bool tol_ok, const void *x0_dev, long long ld0, const void *vectors_dev,
                            long long ld, cfs_hip_sym_t hb = nullptr) {
  int rc = check_lobpcg(h, k, 0, tol_ok, x0_dev, ld0, vectors_dev, ld, a, hb);
  if (rc || (rc = check_whole_matrix(h, not_a_shard("lobpcg_amg"), true, "lobpcg_amg: the whole matrix on one device, not a multi-device handle")))
    return rc;
  if (a->fine != h) return set_err(CFS_HIP_ERR_ARG, "lobpcg_amg: the hierarchy was created on another handle");
  if (a->is_stale()) return set_err(CFS_HIP_ERR_ARG, "lobpcg_amg: the last refresh failed");
  return 0;
}

int cfs_hip_sym_lobpcg_amg(cfs_hip_sym_t h, cfs_hip_amg_t a, int k, double tol, double scale, int maxiter, const void *x0_dev, long long ld0,
                           double *eigenvalues, void *vectors_dev, long long ld, double *residuals, int *nconv, int *iterations,
                           int *products, void *stream) {
  if (!h || !a || !eigenvalues || !vectors_dev) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (nconv) *nconv = 0;
  if (iterations) *iterations = 0;
  if (products) *products = 0;
  const bool tol_ok = tol >= 0.0 && scale > 0.0 && std::isfinite(scale) && maxiter >= 0;
  int rc = check_lobpcg_amg(h, a, k, tol_ok, x0_dev, ld0, vectors_dev, ld);
  if (rc) return rc;
  h->ok_x = h->ok_y = nullptr;
  DeviceGuard g(h->device);
  return a->lobpcg(nullptr, k, tol, scale, maxiter, -1, x0_dev, ld0, eigenvalues, vectors_dev, ld, residuals, nconv, iterations, products,
                   nullptr, (hipStream_t)stream);
}

int cfs_hip_sym_debug_lobpcg_amg(cfs_hip_sym_t h, cfs_hip_amg_t a, int k, const void *x0_dev, long long ld0, int iters, double *theta,
                                 void *vectors_dev, long long ld, double *resnorms, void *stream) {
  if (!h || !a || !theta || !vectors_dev || !resnorms) return set_err(CFS_HIP_ERR_ARG, "null argument");
  int rc = check_lobpcg_amg(h, a, k, iters >= 0, x0_dev, ld0, vectors_dev, ld);
  if (rc) return rc;
  h->ok_x = h->ok_y = nullptr;
  DeviceGuard g(h->device);
  return a->lobpcg(nullptr, k, 0.0, 1.0, 0, iters, x0_dev, ld0, theta, vectors_dev, ld, resnorms, nullptr, nullptr, nullptr, nullptr,
                   (hipStream_t)stream);
}

// ---- LOBPCG for the pencil A x = lambda B x: the same templates with the third block B S ----
int cfs_hip_sym_lobpcg_gen(cfs_hip_sym_t h, cfs_hip_sym_t hb, int k, int block_rows, double tol, double scale, int maxiter,
                           const void *x0_dev, long long ld0, double *eigenvalues, void *vectors_dev, long long ld, double *residuals,
                           int *nconv, int *iterations, int *products, int *b_products, void *stream) {
  if (!h || !hb || !eigenvalues || !vectors_dev) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (nconv) *nconv = 0;
  if (iterations) *iterations = 0;
  if (products) *products = 0;
  if (b_products) *b_products = 0;
  const bool tol_ok = tol >= 0.0 && scale > 0.0 && std::isfinite(scale) && maxiter >= 0;
  int rc = check_lobpcg(h, k, block_rows, tol_ok, x0_dev, ld0, vectors_dev, ld, nullptr, hb);
  if (rc) return rc;
  h->ok_x = h->ok_y = hb->ok_x = hb->ok_y = nullptr; // (the iteration's own vectors are library memory on the handles' device)
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::lobpcg<decltype(v), decltype(bs)::value, true>(h, hb, k, tol, scale, maxiter, -1, x0_dev, ld0, eigenvalues, vectors_dev,
                                                                      ld, residuals, nconv, iterations, products, b_products, st);
  });
}

int cfs_hip_sym_debug_lobpcg_gen(cfs_hip_sym_t h, cfs_hip_sym_t hb, int k, int block_rows, const void *x0_dev, long long ld0, int iters,
                                 double *theta, void *vectors_dev, long long ld, double *resnorms, void *stream) {
  if (!h || !hb || !theta || !vectors_dev || !resnorms) return set_err(CFS_HIP_ERR_ARG, "null argument");
  int rc = check_lobpcg(h, k, block_rows, iters >= 0, x0_dev, ld0, vectors_dev, ld, nullptr, hb);
  if (rc) return rc;
  h->ok_x = h->ok_y = hb->ok_x = hb->ok_y = nullptr;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::lobpcg<decltype(v), decltype(bs)::value, true>(h, hb, k, 0.0, 1.0, 0, iters, x0_dev, ld0, theta, vectors_dev, ld,
                                                                      resnorms, nullptr, nullptr, nullptr, nullptr, st);
  });
}

int cfs_hip_sym_lobpcg_gen_amg(cfs_hip_sym_t h, cfs_hip_sym_t hb, cfs_hip_amg_t a, int k, double tol, double scale, int maxiter,
                               const void *x0_dev, long long ld0, double *eigenvalues, void *vectors_dev, long long ld, double *residuals,
                               int *nconv, int *iterations, int *products, int *b_products, void *stream) {
  if (!h || !hb || !a || !eigenvalues || !vectors_dev) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (nconv) *nconv = 0;
  if (iterations) *iterations = 0;
  if (products) *products = 0;
  if (b_products) *b_products = 0;
  const bool tol_ok = tol >= 0.0 && scale > 0.0 && std::isfinite(scale) && maxiter >= 0;
  int rc = check_lobpcg_amg(h, a, k, tol_ok, x0_dev, ld0, vectors_dev, ld, hb);
  if (rc) return rc;
  h->ok_x = h->ok_y = hb->ok_x = hb->ok_y = nullptr;
  DeviceGuard g(h->device);
  return a->lobpcg(hb, k, tol, scale, maxiter, -1, x0_dev, ld0, eigenvalues, vectors_dev, ld, residuals, nconv, iterations, products,
                   b_products, (hipStream_t)stream);
}

int cfs_hip_debug_lobpcg_rr(int m, const double *g, const double *hh, int k, double drop, double *theta, double *c, int *rank) {
  if (!g || !hh || !theta || !c || !rank) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (m < 1 || m > 3 * CFS_HIP_LOBPCG_MAX_K || k < 1 || k > CFS_HIP_LOBPCG_MAX_K || k > m)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_rr: 1 <= m <= " + std::to_string(3 * CFS_HIP_LOBPCG_MAX_K) + " and 1 <= k <= min(m, " +
                                        std::to_string(CFS_HIP_LOBPCG_MAX_K) + ")");
  if (!(drop >= 0.0) || !(drop < 1.0)) return set_err(CFS_HIP_ERR_ARG, "lobpcg_rr: the drop threshold must lie in [0, 1)");
  if (cfs_solver::lobpcg_rr(m, g, hh, k, drop, theta, c, rank) < 0)
    return set_err(CFS_HIP_ERR_INTERNAL, "lobpcg_rr: entries that are not finite, or no convergence");
  return 0;
}

// the device blocks of the kernel-level developer entry points: 16-byte aligned (checked for every block first) device
// memory, one device
static int check_lobpcg_geom(const void *p, long long ld, long long n, int value_bytes, const char *who) {
  if (value_bytes != 4 && value_bytes != 8) return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": value_bytes must be 4 or 8");
  // (the upper limit keeps the byte span of a block within 63 bits)
  if (n < 1 || ld < n || ld > (1LL << 62) / (8LL * 3 * CFS_HIP_LOBPCG_MAX_K) || (ld * value_bytes) % 16 != 0 || ((uintptr_t)p & 15))
    return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": n >= 1, ld >= n, the pointers and ld multiples of 16 bytes");
  return 0;
}
static int check_lobpcg_dev(const void *p, const char *who, int *dev) {
  const cfs_rt::PtrInfo pi = cfs_rt::classify(p);
  if (!pi.device) return set_err(CFS_HIP_ERR_ARG, std::string(who) + " needs device pointers");
  if (*dev >= 0 && pi.dev != *dev) return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": the blocks live on different devices");
  *dev = pi.dev;
  return 0;
}

// a column list of the kernel-level entry points: idx[j] in [0, ncols)
static int check_lobpcg_idx(const int *idx, int m, int ncols, const char *who) {
  for (int j = 0; j < m; ++j)
    if (idx[j] < 0 || idx[j] >= ncols)
      return set_err(CFS_HIP_ERR_ARG, std::string(who) + ": idx[" + std::to_string(j) + "] = " + std::to_string(idx[j]) +
                                          " is not a column in [0, " + std::to_string(ncols) + ")");
  return 0;
}

int cfs_hip_debug_gram_cols(const void *s_dev, const void *t_dev, long long ld, long long n, int m, const int *idx, int full_h,
                            int value_bytes, double *g, double *hh, void *stream) {
  if (!s_dev || !t_dev || !idx || !g || !hh) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (m < 1 || m > 3 * CFS_HIP_LOBPCG_MAX_K)
    return set_err(CFS_HIP_ERR_ARG, "gram: m must lie in [1, " + std::to_string(3 * CFS_HIP_LOBPCG_MAX_K) + "]");
  int dev = -1, rc;
  if ((rc = check_lobpcg_idx(idx, m, 3 * CFS_HIP_LOBPCG_MAX_K, "gram"))) return rc;
  if (full_h != 0 && full_h != 1) return set_err(CFS_HIP_ERR_ARG, "gram: full_h must be 0 or 1");
  if ((rc = check_lobpcg_geom(s_dev, ld, n, value_bytes, "gram")) || (rc = check_lobpcg_geom(t_dev, ld, n, value_bytes, "gram")) ||
      (rc = check_lobpcg_dev(s_dev, "gram", &dev)) || (rc = check_lobpcg_dev(t_dev, "gram", &dev)))
    return rc;
  DeviceGuard dg(dev);
  return cfs_rt::with_value_type(value_bytes, [&](auto v) {
    return cfs_solver::debug_gram<decltype(v)>(s_dev, t_dev, nullptr, ld, n, m, idx, full_h, g, hh, (hipStream_t)stream);
  });
}

int cfs_hip_debug_gram(const void *s_dev, const void *t_dev, long long ld, long long n, int m, int value_bytes, double *g, double *hh,
                       void *stream) {
  int idx[3 * CFS_HIP_LOBPCG_MAX_K];
  for (int j = 0; j < 3 * CFS_HIP_LOBPCG_MAX_K; ++j) idx[j] = j;
  return cfs_hip_debug_gram_cols(s_dev, t_dev, ld, n, m, idx, 1, value_bytes, g, hh, stream);
}

int cfs_hip_debug_lobpcg_update_cols(void *s_dev, void *as_dev, long long ld, long long n, int k, int m, const int *idx, int with_p,
                                     const double *c, int value_bytes, void *stream) {
  if (!s_dev || !idx || !c) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (k < 1 || k > CFS_HIP_LOBPCG_MAX_K || m < 1 || m > 3 * k)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_update: 1 <= k <= " + std::to_string(CFS_HIP_LOBPCG_MAX_K) + " and 1 <= m <= 3 k");
  int dev = -1, rc;
  if ((rc = check_lobpcg_idx(idx, m, 3 * k, "lobpcg_update"))) return rc;
  if (with_p != 0 && with_p != 1) return set_err(CFS_HIP_ERR_ARG, "lobpcg_update: with_p must be 0 or 1");
  if ((rc = check_lobpcg_geom(s_dev, ld, n, value_bytes, "lobpcg_update")) ||
      (as_dev && (rc = check_lobpcg_geom(as_dev, ld, n, value_bytes, "lobpcg_update"))))
    return rc;
  if (as_dev) {
    // the two blocks, first byte to the last row of the last column, must not overlap
    const uintptr_t span = (uintptr_t)(((long long)(3 * k - 1) * ld + n) * value_bytes), s0 = (uintptr_t)s_dev, a0 = (uintptr_t)as_dev;
    if (s0 < a0 + span && a0 < s0 + span) return set_err(CFS_HIP_ERR_ARG, "lobpcg_update: the two blocks overlap");
  }
  if ((rc = check_lobpcg_dev(s_dev, "lobpcg_update", &dev)) || (as_dev && (rc = check_lobpcg_dev(as_dev, "lobpcg_update", &dev)))) return rc;
  DeviceGuard dg(dev);
  return cfs_rt::with_value_type(value_bytes, [&](auto v) {
    return cfs_solver::debug_update<decltype(v)>(s_dev, as_dev, nullptr, ld, n, k, m, idx, with_p, c, (hipStream_t)stream);
  });
}

int cfs_hip_debug_lobpcg_update(void *s_dev, long long ld, long long n, int k, int m, const double *c, int value_bytes, void *stream) {
  int idx[3 * CFS_HIP_LOBPCG_MAX_K];
  for (int j = 0; j < 3 * CFS_HIP_LOBPCG_MAX_K; ++j) idx[j] = j;
  return cfs_hip_debug_lobpcg_update_cols(s_dev, nullptr, ld, n, k, m, idx, 1, c, value_bytes, stream);
}

// the three-block forms of the pencil solver: the checks of the two-block forms, with the third block among them
int cfs_hip_debug_gram3_cols(const void *s_dev, const void *as_dev, const void *bs_dev, long long ld, long long n, int m, const int *idx,
                             int value_bytes, double *g, double *hh, void *stream) {
  if (!s_dev || !as_dev || !bs_dev || !idx || !g || !hh) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (m < 1 || m > 3 * CFS_HIP_LOBPCG_MAX_K)
    return set_err(CFS_HIP_ERR_ARG, "gram3: m must lie in [1, " + std::to_string(3 * CFS_HIP_LOBPCG_MAX_K) + "]");
  int dev = -1, rc;
  if ((rc = check_lobpcg_idx(idx, m, 3 * CFS_HIP_LOBPCG_MAX_K, "gram3"))) return rc;
  for (const void *p : {s_dev, as_dev, bs_dev})
    if ((rc = check_lobpcg_geom(p, ld, n, value_bytes, "gram3"))) return rc;
  for (const void *p : {s_dev, as_dev, bs_dev})
    if ((rc = check_lobpcg_dev(p, "gram3", &dev))) return rc;
  DeviceGuard dg(dev);
  return cfs_rt::with_value_type(value_bytes, [&](auto v) {
    return cfs_solver::debug_gram<decltype(v)>(s_dev, as_dev, bs_dev, ld, n, m, idx, 0, g, hh, (hipStream_t)stream);
  });
}

int cfs_hip_debug_lobpcg_update3_cols(void *s_dev, void *as_dev, void *bs_dev, long long ld, long long n, int k, int m, const int *idx,
                                      int with_p, const double *c, int value_bytes, void *stream) {
  if (!s_dev || !as_dev || !bs_dev || !idx || !c) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (k < 1 || k > CFS_HIP_LOBPCG_MAX_K || m < 1 || m > 3 * k)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_update3: 1 <= k <= " + std::to_string(CFS_HIP_LOBPCG_MAX_K) + " and 1 <= m <= 3 k");
  int dev = -1, rc;
  if ((rc = check_lobpcg_idx(idx, m, 3 * k, "lobpcg_update3"))) return rc;
  if (with_p != 0 && with_p != 1) return set_err(CFS_HIP_ERR_ARG, "lobpcg_update3: with_p must be 0 or 1");
  for (const void *p : {(const void *)s_dev, (const void *)as_dev, (const void *)bs_dev})
    if ((rc = check_lobpcg_geom(p, ld, n, value_bytes, "lobpcg_update3"))) return rc;
  // the three blocks, first byte to the last row of the last column, must not overlap
  const uintptr_t span = (uintptr_t)(((long long)(3 * k - 1) * ld + n) * value_bytes), b[3] = {(uintptr_t)s_dev, (uintptr_t)as_dev, (uintptr_t)bs_dev};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (b[i] < b[j] + span && b[j] < b[i] + span) return set_err(CFS_HIP_ERR_ARG, "lobpcg_update3: two of the blocks overlap");
  for (const void *p : {(const void *)s_dev, (const void *)as_dev, (const void *)bs_dev})
    if ((rc = check_lobpcg_dev(p, "lobpcg_update3", &dev))) return rc;
  DeviceGuard dg(dev);
  return cfs_rt::with_value_type(value_bytes, [&](auto v) {
    return cfs_solver::debug_update<decltype(v)>(s_dev, as_dev, bs_dev, ld, n, k, m, idx, with_p, c, (hipStream_t)stream);
  });
}

// cfs_hip_sym_debug_lobpcg_residual (bx_dev = NULL) and _residual_gen behind their null checks
static int run_lobpcg_residual(cfs_hip_sym_t h, int block_rows, const void *x_dev, const void *ax_dev, const void *bx_dev, void *w_dev,
                               long long ld, int k, const double *theta, unsigned active, double *sums, void *stream) {
  if (k < 1 || k > CFS_HIP_LOBPCG_MAX_K)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_residual: bad k: 1 <= k <= " + std::to_string(CFS_HIP_LOBPCG_MAX_K) + ", got k = " + std::to_string(k));
  if (block_rows != 0 && !block_rows_ok(block_rows))
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_residual: block_rows " + std::to_string(block_rows) + " is not one of 0, 1, 2, 3, 4, 6");
  if (active >> k) return set_err(CFS_HIP_ERR_ARG, "lobpcg_residual: active names a pair that is not in [0, k)");
  if ((((uintptr_t)x_dev) | ((uintptr_t)ax_dev) | ((uintptr_t)bx_dev) | ((uintptr_t)w_dev)) & 15)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_residual: X, AX and W must be 16-byte aligned");
  if (!h->send_rows().empty() || h->rows() != h->n())
    return set_err(CFS_HIP_ERR_UNSUPPORTED, "lobpcg_residual: a handle of the whole matrix, not a shard");
  const long long n = h->n();
  // (the upper limit keeps the byte spans of k columns within 63 bits)
  if (ld < n || ld > (1LL << 62) / (8LL * CFS_HIP_LOBPCG_MAX_K) || (ld * h->value_bytes) % 16 != 0)
    return set_err(CFS_HIP_ERR_ARG, "lobpcg_residual: bad ld " + std::to_string(ld) + ": at least n = " + std::to_string(n) +
                                        " and a multiple of 16 bytes");
  // W is written while X and AX are read: the k columns of W may not overlap those of X or AX
  const uintptr_t span = (uintptr_t)(((long long)(k - 1) * ld + n) * h->value_bytes), w0 = (uintptr_t)w_dev;
  for (const void *p : {x_dev, ax_dev, bx_dev})
    if (p && (uintptr_t)p < w0 + span && w0 < (uintptr_t)p + span)
      return set_err(CFS_HIP_ERR_ARG, "lobpcg_residual: W overlaps X or AX");
  if (block_rows >= 2) {
    int ngpus = 1;
    if (cfs_hip_sym_num_gpus(h, &ngpus) == 0 && ngpus != 1)
      return set_err(CFS_HIP_ERR_UNSUPPORTED, "lobpcg_residual: block Jacobi needs the whole matrix on one device (blocks straddle the "
                                              "row splits of a multi-device handle)");
  }
  int rc;
  if ((rc = check_eigs_ptr(h, x_dev, "lobpcg_residual", "X")) || (rc = check_eigs_ptr(h, ax_dev, "lobpcg_residual", "AX")) ||
      (bx_dev && (rc = check_eigs_ptr(h, bx_dev, "lobpcg_residual", "BX"))) || (rc = check_eigs_ptr(h, w_dev, "lobpcg_residual", "W")))
    return rc;
  h->ok_x = h->ok_y = nullptr;
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return with_precond(h->value_bytes, block_rows, [&](auto v, auto bs) {
    return cfs_solver::debug_residual<decltype(v), decltype(bs)::value>(h, x_dev, ax_dev, bx_dev, w_dev, ld, k, theta, active, sums, st);
  });
}

int cfs_hip_sym_debug_lobpcg_residual(cfs_hip_sym_t h, int block_rows, const void *x_dev, const void *ax_dev, void *w_dev, long long ld,
                                      int k, const double *theta, unsigned active, double *sums, void *stream) {
  if (!h || !x_dev || !ax_dev || !w_dev || !theta || !sums) return set_err(CFS_HIP_ERR_ARG, "null argument");
  return run_lobpcg_residual(h, block_rows, x_dev, ax_dev, nullptr, w_dev, ld, k, theta, active, sums, stream);
}

int cfs_hip_sym_debug_lobpcg_residual_gen(cfs_hip_sym_t h, int block_rows, const void *x_dev, const void *ax_dev, const void *bx_dev,
                                          void *w_dev, long long ld, int k, const double *theta, unsigned active, double *sums,
                                          void *stream) {
  if (!h || !x_dev || !ax_dev || !bx_dev || !w_dev || !theta || !sums) return set_err(CFS_HIP_ERR_ARG, "null argument");
  return run_lobpcg_residual(h, block_rows, x_dev, ax_dev, bx_dev, w_dev, ld, k, theta, active, sums, stream);
}

int cfs_hip_sym_spmv(cfs_hip_sym_t h, void *y, const void *x) {
  if (!h || !y || !x) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (!h->send_rows().empty())
    return set_err(CFS_HIP_ERR_ARG, "sharded handle: use cfs_hip_sym_spmv_local_async");
  const size_t vb = (size_t)h->value_bytes;
  return run_staged(h->device, h->stage, (size_t)h->n() * vb, (size_t)h->rows() * vb, y, x,
                    [&](void *yd, const void *xd, hipStream_t st) {
                      return h->spmv_local(yd, xd, nullptr, st);
                    });
}

// New numeric values, same sparsity pattern (a matrix reassembled in every step of a
// non-linear solve): the caller's full CSR value array -- host or device pointer -- is
// poured into the existing schedule by a device kernel; tune() is not repeated.
static int update_values(cfs_hip_sym_t h, const void *values, long long nnz, size_t vb) {
  if (!h || !values) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if ((size_t)h->value_bytes != vb) return set_err(CFS_HIP_ERR_ARG, "value type differs from the handle's");
  cfs_rt::DevCtx *ctx;
  int rc = cfs_rt::device_ctx(h->device, &ctx);
  if (rc) return rc;
  DeviceGuard g(h->device);
  const cfs_rt::PtrInfo vi = cfs_rt::classify(values);
  DevBuf tmp;
  const void *src = values;
  if (!vi.device) {
    if ((rc = tmp.alloc((size_t)nnz * vb))) return rc;
    HIPCHK(hipMemcpyAsync(tmp.p, values, (size_t)nnz * vb, hipMemcpyHostToDevice, ctx->stream));
    src = tmp.p;
  } else if (vi.dev != h->device) {
    return set_err(CFS_HIP_ERR_ARG, "values live on another device than the matrix");
  }
  if ((rc = h->update_values(src, nnz, ctx->stream))) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream)); // tmp goes away; later SpMVs on any stream see the values
  return 0;
}
int cfs_hip_sym_update_values_f64(cfs_hip_sym_t h, const double *values, long long nnz) {
  return update_values(h, values, nnz, 8);
}
int cfs_hip_sym_update_values_f32(cfs_hip_sym_t h, const float *values, long long nnz) {
  return update_values(h, values, nnz, 4);
}

int cfs_hip_sym_shard_send_counts(cfs_hip_sym_t h, int *send_counts) {
  if (!h || !send_counts) return set_err(CFS_HIP_ERR_ARG, "null argument");
  const auto &c = h->send_counts();
  for (size_t i = 0; i < c.size(); i++) send_counts[i] = c[i];
  return 0;
}
int cfs_hip_sym_shard_send_rows(cfs_hip_sym_t h, int *rows) {
  if (!h || !rows) return set_err(CFS_HIP_ERR_ARG, "null argument");
  const auto &r = h->send_rows();
  for (size_t i = 0; i < r.size(); i++) rows[i] = r[i];
  return 0;
}
int cfs_hip_sym_shard_set_recv(cfs_hip_sym_t h, int nrecv, const int *recv_rows) {
  if (!h || (nrecv > 0 && !recv_rows)) return set_err(CFS_HIP_ERR_ARG, "null argument");
  return h->set_recv(nrecv, recv_rows);
}
int cfs_hip_sym_spmv_local_async(cfs_hip_sym_t h, void *y, const void *x, void *send,
                                 void *stream) {
  if (!h || !y || !x) return set_err(CFS_HIP_ERR_ARG, "null argument");
  int rc = check_placement(h, y, x);
  if (rc) return rc;
  DeviceGuard g(h->device);
  return h->spmv_local(y, x, send, (hipStream_t)stream);
}
int cfs_hip_sym_spmv_phases_async(cfs_hip_sym_t h, void *y, const void *x, void *send,
                                  int phases, void *stream) {
  if (!h || !y || !x) return set_err(CFS_HIP_ERR_ARG, "null argument");
  int rc = check_placement(h, y, x);
  if (rc) return rc;
  DeviceGuard g(h->device);
  return h->spmv_local(y, x, send, (hipStream_t)stream, phases);
}
int cfs_hip_sym_recv_fold_async(cfs_hip_sym_t h, void *y, const void *recv, void *stream) {
  if (!h || !y) return set_err(CFS_HIP_ERR_ARG, "null argument");
  DeviceGuard g(h->device);
  return h->recv_fold(y, recv, (hipStream_t)stream);
}

int cfs_hip_sym_debug_timeline(cfs_hip_sym_t h, void *y_dev, const void *x_dev,
                               unsigned long long *stamps, int capacity_words, int *ngroups) {
  if (!h || !y_dev || !x_dev || !stamps || !ngroups) return set_err(CFS_HIP_ERR_ARG, "null argument");
  return h->timeline(y_dev, x_dev, stamps, capacity_words, ngroups);
}

int cfs_hip_sym_debug_group_features(cfs_hip_sym_t h, long long *out, int capacity_words,
                                     int *ngroups) {
  if (!h || !out || !ngroups) return set_err(CFS_HIP_ERR_ARG, "null argument");
  return h->group_features(out, capacity_words, ngroups);
}

int cfs_hip_sym_get_stats(cfs_hip_sym_t h, cfs_hip_sym_stats *out) {
  if (!h || !out) return set_err(CFS_HIP_ERR_ARG, "null argument");
  h->stats(out);
  return 0;
}

// developer / test: digests of the schedule's device arrays (cfs_hip.h)
static unsigned long long fnv1a(const void *p, size_t n, unsigned long long h = 1469598103934665603ull) {
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
template <typename V> static int sym_digest(SymMatrix<V> *m, unsigned long long *w) {
  DeviceGuard g(m->device);
  HIPCHK(hipDeviceSynchronize());
  std::vector<unsigned char> buf;
  auto dig = [&](const DevBuf &b, size_t bytes, unsigned long long *out) -> int {
    *out = 0;
    if (!b.p || bytes == 0) return 0;
    buf.resize(bytes);
    HIPCHK(hipMemcpy(buf.data(), b.p, bytes, hipMemcpyDeviceToHost));
    *out = fnv1a(buf.data(), bytes);
    return 0;
  };
  const SymPlan<V> &P = m->P;
  const size_t T = P.tiles.size(), G = P.group_first.size(), s = sizeof(V);
  int64_t nsl = 0, nvr = 0;
  for (const Tile &t : P.tiles) nsl += t.nslots, nvr += t.nvrows;
  int rc, k = 0;
  { // tiles, aexp masked (the device builder does not compute it: the deterministic build only)
    std::vector<Tile> tt(T);
    if (T) HIPCHK(hipMemcpy(tt.data(), m->tiles.p, T * sizeof(Tile), hipMemcpyDeviceToHost));
    for (auto &t : tt) t.aexp = 0;
    w[k++] = fnv1a(tt.data(), T * sizeof(Tile));
    std::vector<Tile> gf(G);
    if (G) HIPCHK(hipMemcpy(gf.data(), m->gfirst.p, G * sizeof(Tile), hipMemcpyDeviceToHost));
    for (auto &t : gf) t.aexp = 0;
    w[k++] = fnv1a(gf.data(), G * sizeof(Tile));
  }
  if ((rc = dig(m->group_ptr, G * sizeof(int2), &w[k++]))) return rc;
  if ((rc = dig(m->slot_col, (size_t)nsl * 4, &w[k++]))) return rc;
  if ((rc = dig(m->rowinfo, (size_t)nvr * 4, &w[k++]))) return rc;
  if ((rc = dig(m->diag, (size_t)nvr * s, &w[k++]))) return rc;
  if ((rc = dig(m->slice_meta, (size_t)m->nslices * 16, &w[k++]))) return rc;
  if ((rc = dig(m->leadlane, (size_t)m->nslices * 64, &w[k++]))) return rc;
  if ((rc = dig(m->vals, (size_t)m->stream_len * s, &w[k++]))) return rc;
  if ((rc = dig(m->slots, (size_t)m->slot_len * 2, &w[k++]))) return rc;
  if ((rc = dig(m->cvals, (size_t)m->coo_len * s, &w[k++]))) return rc;
  if ((rc = dig(m->crows, (size_t)m->coo_len * 2, &w[k++]))) return rc;
  if ((rc = dig(m->ccols, (size_t)m->coo_len * 2, &w[k++]))) return rc;
  if ((rc = dig(m->fold_rec, (size_t)(m->nfold + 1) * sizeof(int4), &w[k++]))) return rc;
  if ((rc = dig(m->fold_idx, m->fold_idx.bytes, &w[k++]))) return rc;
  if ((rc = dig(m->val_map, m->has_value_map ? (size_t)m->stream_len * 4 : 0, &w[k++]))) return rc;
  if ((rc = dig(m->cval_map, m->has_value_map ? (size_t)m->coo_len * 4 : 0, &w[k++]))) return rc;
  if ((rc = dig(m->diag_map, m->has_value_map ? (size_t)nvr * 4 : 0, &w[k++]))) return rc;
  w[k++] = (unsigned long long)m->P.lds_slots | ((unsigned long long)m->P.ngroups << 32);
  if ((rc = dig(m->slot_exp, m->P.deterministic ? (size_t)nsl * 2 : 0, &w[k++]))) return rc;
  if ((rc = dig(m->send_ptr, m->nsend > 0 ? ((size_t)m->nsend + 1) * 4 : 0, &w[k++]))) return rc;
  if ((rc = dig(m->send_idx, m->nsend > 0 ? (size_t)m->P.send_ptr.back() * 4 : 0, &w[k++]))) return rc;
  { // far sections (Format::hyb)
    const size_t fl = (size_t)P.far_len;
    if ((rc = dig(m->fvals, fl * s, &w[k++]))) return rc;
    if ((rc = dig(m->frows, fl * 2, &w[k++]))) return rc;
    if ((rc = dig(m->fcols, fl * 4, &w[k++]))) return rc;
    if ((rc = dig(m->fval_map, m->has_value_map ? fl * 4 : 0, &w[k++]))) return rc;
    w[k++] = (unsigned long long)P.far_entries;
  }
  w[CFS_HIP_DIGEST_WORDS - 1] = m->device_built ? 1ull : 0ull;
  return 0;
}
template <typename V> static int sym_kernel(const SymMatrix<V> *m, int *w) {
  const auto t = m->tile_variant();
  const int v[CFS_HIP_KERNEL_WORDS] = {(int)sizeof(V), t.block, t.mode, t.nt, t.offb, t.u, t.det, t.comb};
  for (int i = 0; i < CFS_HIP_KERNEL_WORDS; i++) w[i] = v[i];
  return 0;
}
int cfs_hip_sym_debug_kernel(cfs_hip_sym_t h, int *words, int capacity_words) {
  if (!h || !words || capacity_words < CFS_HIP_KERNEL_WORDS) return set_err(CFS_HIP_ERR_ARG, "bad argument");
  if (auto *d = dynamic_cast<SymMatrix<double> *>(h)) return sym_kernel<double>(d, words);
  if (auto *f = dynamic_cast<SymMatrix<float> *>(h)) return sym_kernel<float>(f, words);
  return set_err(CFS_HIP_ERR_ARG, "no single tile kernel for a multi-device handle");
}
int cfs_hip_sym_debug_plan_note(cfs_hip_sym_t h, char *buf, int capacity) {
  if (!h || !buf || capacity < 1) return set_err(CFS_HIP_ERR_ARG, "bad argument");
  snprintf(buf, (size_t)capacity, "%s", h->plan_note.c_str());
  return 0;
}
int cfs_hip_sym_debug_digest(cfs_hip_sym_t h, unsigned long long *words, int capacity_words) {
  if (!h || !words || capacity_words < CFS_HIP_DIGEST_WORDS) return set_err(CFS_HIP_ERR_ARG, "bad argument");
  for (int i = 0; i < CFS_HIP_DIGEST_WORDS; i++) words[i] = 0;
  if (auto *d = dynamic_cast<SymMatrix<double> *>(h)) return sym_digest<double>(d, words);
  if (auto *f = dynamic_cast<SymMatrix<float> *>(h)) return sym_digest<float>(f, words);
  return set_err(CFS_HIP_ERR_ARG, "no digest for a multi-device handle");
}
// developer / test: the lists cfs_fold_kernel walks, decoded from the device arrays (cfs_hip.h)
template <typename V>
static int sym_fold_lists(SymMatrix<V> *m, int which, int *dst, int *len, int capacity, int *count) {
  DeviceGuard g(m->device);
  HIPCHK(hipDeviceSynchronize());
  const DevBuf &rb = which ? m->rfold_rec : m->fold_rec, &ib = which ? m->rfold_idx : m->fold_idx;
  const int nf = which ? m->nrfold : m->nfold;
  *count = nf;
  if (nf == 0) return 0;
  if (capacity < nf) return set_err(CFS_HIP_ERR_ARG, "buffer too small: one entry per fold destination");
  std::vector<int4> rec((size_t)nf);
  std::vector<int32_t> rest(ib.bytes / 4);
  HIPCHK(hipMemcpy(rec.data(), rb.p, rec.size() * sizeof(int4), hipMemcpyDeviceToHost));
  if (!rest.empty()) HIPCHK(hipMemcpy(rest.data(), ib.p, rest.size() * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < nf; i++) {
    const int4 r = rec[(size_t)i];
    dst[i] = r.x;
    if (r.w >= -1) {
      len[i] = 1 + (r.z >= 0) + (r.w >= 0);
    } else { // e2 = -(offset + 2): [count, entries 2..] in the remainder list
      const size_t off = (size_t)(-(r.w + 2));
      if (off >= rest.size() || rest[off] < 0 || off + 1 + (size_t)rest[off] > rest.size())
        return set_err(CFS_HIP_ERR_INTERNAL, "fold record " + std::to_string(i) + " points outside the remainder lists");
      len[i] = 2 + rest[off];
    }
  }
  return 0;
}
int cfs_hip_sym_debug_fold_lists(cfs_hip_sym_t h, int which, int *dst, int *len, int capacity, int *count) {
  if (!h || !count || (which != 0 && which != 1) || capacity < 0 || (capacity > 0 && (!dst || !len)))
    return set_err(CFS_HIP_ERR_ARG, "bad argument");
  if (auto *d = dynamic_cast<SymMatrix<double> *>(h)) return sym_fold_lists<double>(d, which, dst, len, capacity, count);
  if (auto *f = dynamic_cast<SymMatrix<float> *>(h)) return sym_fold_lists<float>(f, which, dst, len, capacity, count);
  return set_err(CFS_HIP_ERR_ARG, "no fold lists for a multi-device handle");
}

// ---- host-only plan self-check (no device needed) -------------------------
template <typename V>
static int plan_check(int n, const int *rowptr, const int *colind, const V *values,
                      int nranks, int rank, const int *row_splits,
                      const cfs_hip_options *opt, cfs_hip_plan_report *rep) {
  if (!rep) return set_err(CFS_HIP_ERR_ARG, "report is NULL");
  memset(rep, 0, sizeof *rep);
  if (n < 0 || !rowptr || (n > 0 && rowptr[n] > 0 && (!colind || !values)))
    return set_err(CFS_HIP_ERR_ARG, "null CSR array");
  if (nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !row_splits))
    return set_err(CFS_HIP_ERR_ARG, "bad rank / nranks / row_splits");
  SymPlan<V> P;
  if (!cfs_plan::build_plan<V>(n, rowptr, colind, values, nranks, rank,
                               nranks > 1 ? row_splits : nullptr, to_opts(opt), P))
    return set_err(plan_error_code(P.error), P.error);
  std::vector<int32_t> r, c, fr, fc, ur, uc;
  std::vector<V> v, fv, uv;
  cfs_plan::decode_plan(P, r, c, v, &fr, &fc, &fv, &ur, &uc, &uv);
  rep->ntiles = (int)P.tiles.size();
  rep->ngroups = P.ngroups;
  rep->nslices = (int64_t)P.slice_meta.size();
  rep->halo_slots = P.nhalo;
  rep->stream_len = P.stream_len;
  rep->nnz_low = P.nnz_low;
  rep->lds_slots = P.lds_slots;
  rep->fold_rows = (int64_t)P.fold_row.size();
  rep->remote_vals = (int64_t)P.send_row.size();
  rep->decoded = (int64_t)r.size();
  rep->far_entries = P.far_entries;
  // (1) decoded triples == strict lower triangle of the owned rows, as
  // multisets of (row, col, value bits): clustering moves an entry to the row
  // of its later end and back, and reorders entries inside rows
  int64_t bad = 0;
  {
    struct Tr {
      int32_t r, c;
      uint64_t v;
      bool operator<(const Tr &o) const {
        return r != o.r ? r < o.r : (c != o.c ? c < o.c : v < o.v);
      }
      bool operator!=(const Tr &o) const { return r != o.r || c != o.c || v != o.v; }
    };
    auto bits = [](V x) {
      uint64_t u = 0;
      memcpy(&u, &x, sizeof(V));
      return u;
    };
    { // HYB: the mirrored far entries are exactly the far entries of the lower side
      std::vector<Tr> F, U;
      for (size_t k = 0; k < fr.size(); k++) F.push_back(Tr{fr[k], fc[k], bits(fv[k])});
      for (size_t k = 0; k < ur.size(); k++) U.push_back(Tr{ur[k], uc[k], bits(uv[k])});
      std::sort(F.begin(), F.end());
      std::sort(U.begin(), U.end());
      if (F.size() != U.size() || (int64_t)F.size() != P.far_entries) bad++;
      for (size_t k = 0; k < std::min(F.size(), U.size()); k++)
        if (F[k] != U[k]) bad++;
    }
    std::vector<Tr> A, B;
    A.reserve(r.size());
    B.reserve(r.size());
    for (size_t k = 0; k < r.size(); k++) A.push_back(Tr{r[k], c[k], bits(v[k])});
    auto lower_pos = [&](int hi, int lo) {
      for (int q = rowptr[hi]; q < rowptr[hi + 1]; q++)
        if (colind[q] == lo) return q;
      return -1;
    };
    int64_t mirrored = 0;
    for (int i = P.row_begin; i < P.row_end; i++)
      for (int j = rowptr[i]; j < rowptr[i + 1]; j++) {
        if (colind[j] < i) B.push_back(Tr{i, colind[j], bits(values[j])});
        else if (P.mirrored && colind[j] >= P.row_end) {
          // mirrored shard: the entry (c, i) of a higher rank's row c, with the
          // value of the LOWER triangle
          const int q = lower_pos(colind[j], i);
          if (q < 0) bad++;
          else B.push_back(Tr{colind[j], i, bits(values[q])});
          mirrored++;
        }
      }
    if (mirrored != P.mirror_entries) bad++;
    rep->mirror_entries = P.mirror_entries;
    // y window classes: slots [nown, ny) are in-block columns, [ny, nslots) are not
    for (const Tile &t : P.tiles) {
      if (t.ny < t.nown || t.ny > t.nslots) bad++;
      for (int h = 0; h < t.nslots - t.nown; h++) {
        const int c = P.halo_col[t.halo_off + h];
        const bool inblock = c >= P.row_begin && c < P.row_end;
        // mirrored shard: exactly the in-block columns have a y window entry;
        // exchange form / whole matrix: every slot has one, no column right of the block
        if (P.mirrored ? inblock != (t.nown + h < t.ny) : (t.ny != t.nslots || c >= P.row_end)) bad++;
      }
    }
    if (P.mirrored && !P.send_row.empty()) bad++;
    std::sort(A.begin(), A.end());
    std::sort(B.begin(), B.end());
    if (A.size() != B.size()) bad += 1 + (int64_t)(A.size() > B.size() ? A.size() - B.size() : B.size() - A.size());
    for (size_t k = 0; k < std::min(A.size(), B.size()); k++)
      if (A[k] != B[k]) bad++;
    // every own row appears exactly once in the slot table, at its diagonal slot
    std::vector<char> seen_row(P.row_end - P.row_begin, 0);
    for (const Tile &t : P.tiles)
      for (int i = 0; i < t.nown; i++) {
        int o = P.slot_col[t.slot_off + i] - P.row_begin;
        if (o < 0 || o >= P.row_end - P.row_begin || seen_row[o]++) bad++;
      }
    for (char ch : seen_row)
      if (!ch) bad++;
  }
  // (1b) CFS_HIP_FLAG_KEEP_VALUE_MAP: every stored value is the caller's value at its
  // recorded position, and every stored entry has a position
  if (!P.val_map.empty()) {
    auto same = [&](const auto &arr, const auto &map, int64_t *mapped) {
      for (size_t k = 0; k < map.size() && k < arr.size(); k++) {
        if (map[k] < 0) continue;
        (*mapped)++;
        if (map[k] >= rowptr[n] || memcmp(&arr[k], &values[map[k]], sizeof(V)) != 0) bad++;
      }
    };
    int64_t mv = 0, mc = 0, mf = 0, md = 0;
    same(P.vals, P.val_map, &mv);
    same(P.cvals, P.cval_map, &mc);
    same(P.fvals, P.fval_map, &mf);
    same(P.diag, P.diag_map, &md);
    if (mv + mc != P.nnz_low + P.mirror_entries - P.far_entries || mf != 2 * P.far_entries) bad++;
    if (md > (int64_t)(P.row_end - P.row_begin)) bad++;
  }
  // (1c) sibling chains (leadlane bits 6 / 7), what entry_combined relies on: a lane that
  // hands its products to its left neighbour is a follower, shares that neighbour's group
  // and row of 16 lanes, has no more packets than it; runs hold at most three lanes; bit 7
  // of a lane mirrors bit 6 of the next one
  for (const Tile &t : P.tiles)
    for (int sidx = 0; sidx < t.nslices; sidx++) {
      const uint8_t *ll = P.leadlane.data() + (size_t)(t.slice_base + sidx) * cfs_plan::kLanes;
      const int p0 = sidx * cfs_plan::kLanes;
      auto packets = [&](int l) {
        return p0 + l < (int)t.nvrows ? (int)(P.rowinfo[t.vrow_off + p0 + l] >> 16) : 0;
      };
      int run = 0;
      for (int l = 0; l < cfs_plan::kLanes; l++) {
        const bool give = ll[l] & 64, take = ll[l] & 128;
        if (give) {
          run++;
          if (l == 0 || (l & 15) == 0 || (ll[l] & 63) == l || (ll[l] & 63) != (ll[l - 1] & 63) ||
              packets(l) > packets(l - 1) || run > 2)
            bad++;
        } else {
          run = 0;
        }
        if (take != (l + 1 < cfs_plan::kLanes && (ll[l + 1] & 64))) bad++;
      }
    }
  // (2) fold + send indices cover every strip entry exactly once and point at
  // a strip entry whose column is the destination row
  {
    std::vector<char> seen((size_t)P.nhalo, 0);
    for (size_t i = 0; i < P.fold_row.size(); i++)
      for (int q = P.fold_ptr[i]; q < P.fold_ptr[i + 1]; q++) {
        int s = P.fold_idx[q];
        if (seen[s]++ || P.halo_col[s] != P.fold_row[i] + P.row_begin) bad++;
      }
    for (size_t i = 0; i < P.send_row.size(); i++)
      for (int q = P.send_ptr[i]; q < P.send_ptr[i + 1]; q++) {
        int s = P.send_idx[q];
        if (seen[s]++ || P.halo_col[s] != P.send_row[i]) bad++;
      }
    int64_t uncovered = 0;
    for (char s : seen)
      if (!s) uncovered++;
    if (uncovered != P.onesided_slots) bad++; // one-sided slots have nothing to fold or send
  }
  // (3) groups partition the tiles; tiles partition the rows
  {
    if (P.group_ptr.front() != 0 || P.group_ptr.back() != (int)P.tiles.size()) bad++;
    if ((int)P.group_ptr.size() != P.ngroups + 1 || P.ngroups % 8) bad++;
    for (size_t g = 1; g < P.group_ptr.size(); g++)
      if (P.group_ptr[g] < P.group_ptr[g - 1]) bad++;
    // every group runs in exactly one launch slot, inside its own XCD's run of slots
    if ((int)P.launch_order.size() != P.ngroups) {
      bad++;
    } else {
      std::vector<char> seen(P.ngroups, 0);
      const int nper = std::max(1, P.ngroups / 8);
      for (int sl = 0; sl < P.ngroups; sl++) {
        const int g = P.launch_order[sl];
        if (g < 0 || g >= P.ngroups || seen[g] || g / nper != sl / nper) {
          bad++;
          continue;
        }
        seen[g] = 1;
      }
    }
    int row = P.row_begin;
    for (const Tile &t : P.tiles) {
      if (t.row0 != row || t.nslots > P.max_slots || t.nslots > P.lds_slots) bad++;
      row += t.nown;
    }
    if (row != P.row_end) bad++;
  }
  rep->mismatches = bad;
  return 0;
}

int cfs_hip_sym_plan_check_f64(int n, const int *rowptr, const int *colind,
                               const double *values, int nranks, int rank,
                               const int *row_splits, const cfs_hip_options *opt,
                               cfs_hip_plan_report *rep) {
  return plan_check<double>(n, rowptr, colind, values, nranks, rank, row_splits, opt, rep);
}
int cfs_hip_sym_plan_check_f32(int n, const int *rowptr, const int *colind,
                               const float *values, int nranks, int rank,
                               const int *row_splits, const cfs_hip_options *opt,
                               cfs_hip_plan_report *rep) {
  return plan_check<float>(n, rowptr, colind, values, nranks, rank, row_splits, opt, rep);
}

int cfs_hip_sym_plan_send_info_f64(int n, const int *rowptr, const int *colind,
                                   const double *values, int nranks, int rank,
                                   const int *row_splits, const cfs_hip_options *opt,
                                   int *send_counts, int *rows, int rows_cap,
                                   int *nrows_out) {
  if (!send_counts || !nrows_out || !row_splits || !rowptr || n < 0 || nranks < 1 || rank < 0 ||
      rank >= nranks)
    return set_err(CFS_HIP_ERR_ARG, "null / bad argument");
  SymPlan<double> P;
  if (!cfs_plan::build_plan<double>(n, rowptr, colind, values, nranks, rank, row_splits,
                                    to_opts(opt), P))
    return set_err(plan_error_code(P.error), P.error);
  for (int r = 0; r < nranks; r++) send_counts[r] = P.send_counts[r];
  *nrows_out = (int)P.send_row.size();
  if (rows) {
    if (rows_cap < *nrows_out) return set_err(CFS_HIP_ERR_ARG, "rows_cap too small");
    for (size_t i = 0; i < P.send_row.size(); i++) rows[i] = P.send_row[i];
  }
  return 0;
}

// ---- plan files (cfs_planfile.hpp is the format; cfs_hip.h the contract) -----------------------
namespace pf = cfs_planfile;

// The file checksum (pf::checksum) of [p, p + bytes) from device memory: a grid-stride loop of
// 16-byte loads (two words each, p 16-byte aligned), a wave reduction, one partial per workgroup;
// the tail of fewer than 16 bytes is read byte by byte by one thread, so nothing outside the range
// is touched.  The sum is an integer sum: any order gives the same bits.
__device__ __forceinline__ unsigned long long cfs_block_sum_u64(unsigned long long s) {
  __shared__ unsigned long long ws[4];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  return ws[0] + ws[1] + ws[2] + ws[3]; // (256 threads = 4 waves)
}
__global__ __launch_bounds__(256) void cfs_checksum_kernel(const unsigned char *__restrict__ p, unsigned long long bytes,
                                                           unsigned long long *__restrict__ partial) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  const unsigned long long nvec = bytes / 16;
  unsigned long long s = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (unsigned long long)gridDim.x * 256) {
    const uint4 v = q[i];
    s += pf::word_term((unsigned long long)v.x | ((unsigned long long)v.y << 32), 2 * i) +
         pf::word_term((unsigned long long)v.z | ((unsigned long long)v.w << 32), 2 * i + 1);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (unsigned long long base = nvec * 16; base < bytes; base += 8) {
      unsigned long long w = 0;
      for (int k = 0; k < 8 && base + k < bytes; k++) w |= (unsigned long long)p[base + k] << (8 * k);
      s += pf::word_term(w, base / 8);
    }
  s = cfs_block_sum_u64(s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void cfs_checksum_final_kernel(const unsigned long long *__restrict__ partial, int n,
                                                                 unsigned long long *__restrict__ out) {
  unsigned long long s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  s = cfs_block_sum_u64(s);
  if (threadIdx.x == 0) *out = s;
}
constexpr int kChecksumGrid = 1024;

// sums[i] = checksum of the device range (ptr[i], bytes[i]), i < count; enqueued on `st`, complete on return
static int device_checksums(const void *const *ptr, const uint64_t *bytes, int count, uint64_t *sums, hipStream_t st) {
  DevBuf scratch; // per range: kChecksumGrid partials; then one result per range
  int rc = scratch.alloc(((size_t)count * kChecksumGrid + (size_t)count) * 8);
  if (rc) return rc;
  unsigned long long *partial = (unsigned long long *)scratch.p, *res = partial + (size_t)count * kChecksumGrid;
  HIPCHK(hipMemsetAsync(res, 0, (size_t)count * 8, st));
  for (int i = 0; i < count; i++) {
    if (bytes[i] == 0) continue;
    if (!ptr[i] || ((uintptr_t)ptr[i] & 15) != 0)
      return set_err(CFS_HIP_ERR_INTERNAL, "internal: checksum of a device array that is not 16-byte aligned");
    const int grid = (int)std::min<uint64_t>((bytes[i] / 16 + 255) / 256 + 1, kChecksumGrid);
    hipLaunchKernelGGL(cfs_checksum_kernel, dim3(grid), dim3(256), 0, st, (const unsigned char *)ptr[i],
                       (unsigned long long)bytes[i], partial + (size_t)i * kChecksumGrid);
    hipLaunchKernelGGL(cfs_checksum_final_kernel, dim3(1), dim3(256), 0, st, partial + (size_t)i * kChecksumGrid, grid, res + i);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sums, res, (size_t)count * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// two page-locked blocks of the pool, an event each and a stream: a file streams through them in
// 16 MiB pieces, the disk side of one piece overlapping the bus side of the other
struct PlanStage {
  static constexpr size_t kPiece = (size_t)16 << 20;
  void *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipStream_t st = nullptr;
  bool used[2] = {false, false};
  int init() {
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
      int rc = cfs_rt::pinned().alloc(kPiece, &pin[k]);
      if (rc) return rc;
      HIPCHK(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    }
    return 0;
  }
  ~PlanStage() {
    if (st) (void)hipStreamSynchronize(st); // nothing may still use the blocks
    for (int k = 0; k < 2; k++) {
      if (ev[k]) (void)hipEventDestroy(ev[k]);
      if (pin[k]) (void)cfs_rt::pinned().release(pin[k]);
    }
    if (st) (void)hipStreamDestroy(st);
  }
};

// the device arrays of a handle in section order (pf::S_TILES .. pf::S_SLOT_EXP)
template <typename V> static void plan_dev_sections(SymMatrix<V> *m, DevBuf **b) {
  DevBuf *const list[pf::kHostFirst] = {&m->tiles, &m->slot_col, &m->rowinfo, &m->diag, &m->slice_meta, &m->leadlane,
                                        &m->vals, &m->slots, &m->cvals, &m->crows, &m->ccols, &m->fvals, &m->frows,
                                        &m->fcols, &m->val_map, &m->cval_map, &m->fval_map, &m->diag_map, &m->fold_rec,
                                        &m->fold_idx, &m->send_ptr, &m->send_idx, &m->slot_exp};
  for (uint32_t i = 0; i < pf::kHostFirst; i++) b[i] = list[i];
}

template <typename V> static int sym_save(SymMatrix<V> *m, const char *path, const char *tag) {
  DeviceGuard g(m->device);
  HIPCHK(hipDeviceSynchronize());
  pf::Extras x;
  x.flags = m->build_flags, x.num_cus = m->num_cus, x.nnz_caller = m->nnz_caller, x.nslices = m->nslices;
  x.combine = m->combine, x.nt_stream = m->nt_stream, x.device_built = m->device_built, x.plan_note = m->plan_note;
  pf::Header h;
  pf::fill_header(m->P, x, tag, m->has_value_map, h);
  DevBuf *dv[pf::kHostFirst];
  plan_dev_sections(m, dv);
  const void *ptr[pf::kSections];
  uint64_t bytes[pf::kSections], sums[pf::kSections];
  uint32_t elem[pf::kSections];
  for (uint32_t i = 0; i < pf::kHostFirst; i++) ptr[i] = dv[i]->p, bytes[i] = dv[i]->p ? dv[i]->bytes : 0;
  for (uint32_t i = pf::kHostFirst; i < pf::kSections; i++) pf::host_section(m->P, i, &ptr[i], &bytes[i]);
  for (uint32_t i = 0; i < pf::kSections; i++) elem[i] = pf::expect(h, i).elem;
  PlanStage s;
  int rc = s.init();
  if (rc) return rc;
  if ((rc = device_checksums(ptr, bytes, (int)pf::kHostFirst, sums, s.st))) return rc;
  for (uint32_t i = pf::kHostFirst; i < pf::kSections; i++) sums[i] = pf::checksum(ptr[i], (size_t)bytes[i]);
  pf::Writer w;
  if (!w.begin(path, h, elem, bytes)) return set_err(CFS_HIP_ERR_FILE, w.error);
  for (uint32_t i = 0; i < pf::kHostFirst; i++) {
    const size_t B = (size_t)bytes[i];
    size_t off = 0, written = 0, plen[2] = {0, 0};
    int k = 0;
    auto issue = [&](int kk) -> int {
      plen[kk] = std::min(PlanStage::kPiece, B - off);
      HIPCHK(hipMemcpyAsync(s.pin[kk], (const char *)ptr[i] + off, plen[kk], hipMemcpyDeviceToHost, s.st));
      HIPCHK(hipEventRecord(s.ev[kk], s.st));
      off += plen[kk];
      return 0;
    };
    if (B && (rc = issue(0))) return rc;
    while (written < B) { // the next piece is on the bus while this one goes to the file
      if (off < B && (rc = issue(k ^ 1))) return rc;
      HIPCHK(hipEventSynchronize(s.ev[k]));
      if (!w.put(i, s.pin[k], plen[k])) return set_err(CFS_HIP_ERR_FILE, w.error);
      written += plen[k];
      k ^= 1;
    }
    if (B == 0 && !w.put(i, nullptr, 0)) return set_err(CFS_HIP_ERR_FILE, w.error);
  }
  for (uint32_t i = pf::kHostFirst; i < pf::kSections; i++)
    if (!w.put(i, ptr[i], (size_t)bytes[i])) return set_err(CFS_HIP_ERR_FILE, w.error);
  if (!w.finish(sums)) return set_err(CFS_HIP_ERR_FILE, w.error);
  return 0;
}

int cfs_hip_sym_save(cfs_hip_sym_t h, const char *path, const char *tag) {
  if (!h || !path) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (tag && strlen(tag) > (size_t)pf::kTagMax) return set_err(CFS_HIP_ERR_ARG, "tag longer than 255 bytes");
  if (auto *d = dynamic_cast<SymMatrix<double> *>(h)) return sym_save<double>(d, path, tag);
  if (auto *f = dynamic_cast<SymMatrix<float> *>(h)) return sym_save<float>(f, path, tag);
  return set_err(CFS_HIP_ERR_UNSUPPORTED, "a multi-device handle cannot be saved: save its shards");
}

template <typename V> static int sym_load(FILE *f, const char *path, const pf::Parsed &F, cfs_hip_sym_t *out) {
  const pf::Header &h = F.h;
  const pf::Scalars &s = h.s;
  auto bad_file = [&](const std::string &what) { return set_err(CFS_HIP_ERR_FILE, std::string(path) + ": " + what); };
  int rc = ensure_init();
  if (rc) return rc;
  int cur_dev = 0;
  HIPCHK(hipGetDevice(&cur_dev));
  std::unique_ptr<SymMatrix<V>> m(new SymMatrix<V>());
  m->value_bytes = (int)sizeof(V);
  m->device = cur_dev;
  SymPlan<V> &P = m->P;
  P.n = (int)s.n, P.row_begin = (int)s.row_begin, P.row_end = (int)s.row_end, P.nranks = (int)s.nranks, P.rank = (int)s.rank;
  P.nnz_low = s.nnz_low, P.nnz_diag = s.nnz_diag, P.nnz_full = s.nnz_full;
  P.max_slots = (int)s.max_slots, P.block_threads = (int)s.block_threads, P.lds_slots = (int)s.lds_slots;
  P.wg_per_cu = (int)s.wg_per_cu, P.deterministic = s.deterministic != 0, P.mirrored = s.mirrored != 0;
  P.ngroups = (int)s.ngroups, P.nvrows = s.nvrows, P.nhalo = s.nhalo, P.onesided_slots = s.onesided_slots;
  P.stream_len = s.stream_len, P.slot_len = s.slot_len, P.coo_len = s.coo_len, P.coo_entries = s.coo_entries;
  P.far_len = s.far_len, P.far_entries = s.far_entries, P.far_candidates = s.far_candidates;
  P.chained_packets = s.chained_packets, P.lane_packets = s.lane_packets, P.mirror_entries = s.mirror_entries;
  // the stored window must fit this device: the check of query_residency, for the stored shape
  {
    const size_t lds = (size_t)P.lds_slots * (size_t)cfs_plan::slot_lds_bytes<V>(P.deterministic);
    int nb = 0;
    if (lds > (size_t)160 * 1024 - 64) nb = 0, rc = 0;
    else if (P.block_threads == 256) rc = residency_one<V, 256>(lds, &nb);
    else if (P.block_threads == 512) rc = residency_one<V, 512>(lds, &nb, P.deterministic);
    else rc = residency_one<V, 1024>(lds, &nb, P.deterministic);
    if (rc) return rc;
    if (nb < 1)
      return set_err(CFS_HIP_ERR_UNSUPPORTED, std::string(path) + ": a window of " + std::to_string(P.lds_slots) + " slots (" +
                                                  std::to_string(lds) + " bytes of LDS, " + std::to_string(P.block_threads) +
                                                  " threads) does not fit this device");
  }
  // the small host arrays (their lengths were checked against the header's counts by pf::parse_file)
  auto read_host = [&](uint32_t id, auto &vec) -> int {
    const pf::Row &r = F.rows[id];
    vec.resize((size_t)(r.bytes / sizeof(vec[0])));
    if (r.bytes && (fseek(f, (long)r.offset, SEEK_SET) != 0 || fread(vec.data(), 1, (size_t)r.bytes, f) != r.bytes))
      return bad_file(std::string("cannot read section ") + pf::section_name(id));
    if (pf::checksum(vec.data(), (size_t)r.bytes) != r.sum)
      return bad_file(std::string("checksum mismatch in section ") + pf::section_name(id));
    return 0;
  };
  if ((rc = read_host(pf::S_GROUP_FIRST, P.group_first)) || (rc = read_host(pf::S_GROUP_PTR, P.group_ptr)) ||
      (rc = read_host(pf::S_LAUNCH_ORDER, P.launch_order)) || (rc = read_host(pf::S_FOLD_DST, P.fold_dst)) ||
      (rc = read_host(pf::S_SEND_ROW, P.send_row)) || (rc = read_host(pf::S_SEND_COUNTS, P.send_counts)) ||
      (rc = read_host(pf::S_TILE_ROUNDS, P.tile_rounds)) || (rc = read_host(pf::S_ROW_SPLITS, P.row_splits)))
    return rc;
  // the device arrays: allocated as DevBuf::upload does (64 zeroed bytes behind the array), the file
  // streamed through the two page-locked blocks
  DevBuf *dv[pf::kHostFirst];
  plan_dev_sections(m.get(), dv);
  PlanStage st;
  if ((rc = st.init())) return rc;
  const void *ptr[pf::kHostFirst];
  uint64_t bytes[pf::kHostFirst], sums[pf::kHostFirst];
  int k = 0;
  for (uint32_t i = 0; i < pf::kHostFirst; i++) {
    const pf::Row &r = F.rows[i];
    DevBuf &b = *dv[i];
    const bool absent = r.bytes == 0 && (i == pf::S_SLOT_EXP || (i >= pf::S_VAL_MAP && i <= pf::S_DIAG_MAP));
    ptr[i] = nullptr, bytes[i] = r.bytes;
    if (absent) continue; // (as after create: no value map, no slot exponents)
    HIPCHK(hipMalloc(&b.p, (size_t)r.bytes + 64));
    b.bytes = (size_t)r.bytes;
    HIPCHK(hipMemsetAsync((char *)b.p + b.bytes, 0, 64, st.st));
    ptr[i] = b.p;
    if (r.bytes && fseek(f, (long)r.offset, SEEK_SET) != 0) return bad_file(std::string("cannot seek to section ") + pf::section_name(i));
    for (size_t off = 0; off < b.bytes; off += PlanStage::kPiece, k ^= 1) {
      const size_t len = std::min(PlanStage::kPiece, b.bytes - off);
      if (st.used[k]) HIPCHK(hipEventSynchronize(st.ev[k]));
      if (fread(st.pin[k], 1, len, f) != len) return bad_file(std::string("cannot read section ") + pf::section_name(i));
      HIPCHK(hipMemcpyAsync((char *)b.p + off, st.pin[k], len, hipMemcpyHostToDevice, st.st));
      HIPCHK(hipEventRecord(st.ev[k], st.st));
      st.used[k] = true;
    }
  }
  // every uploaded array against the table, by the device kernel; nothing of the schedule runs before
  if ((rc = device_checksums(ptr, bytes, (int)pf::kHostFirst, sums, st.st))) return rc;
  for (uint32_t i = 0; i < pf::kHostFirst; i++)
    if (sums[i] != F.rows[i].sum) return bad_file(std::string("checksum mismatch in section ") + pf::section_name(i));
  P.tiles.resize((size_t)s.ntiles);
  if (s.ntiles) HIPCHK(hipMemcpy(P.tiles.data(), m->tiles.p, P.tiles.size() * sizeof(Tile), hipMemcpyDeviceToHost));
  if (s.nsend > 0) {
    P.send_ptr.resize((size_t)s.nsend + 1);
    HIPCHK(hipMemcpy(P.send_ptr.data(), m->send_ptr.p, P.send_ptr.size() * 4, hipMemcpyDeviceToHost));
  }
  m->has_value_map = s.has_value_map != 0;
  m->nnz_caller = s.nnz_caller;
  m->device_built = s.device_built != 0;
  m->plan_note = h.plan_note;
  m->build_flags = (int)s.flags;
  m->num_cus = (int)s.num_cus;
  if (P.deterministic) m->dev_slot_exp = (const short *)m->slot_exp.p;
  if ((rc = m->finish_setup(s.nslices))) return rc;
  // the choices the saved handle had kept (finish_setup applied the size rules and the developer knobs)
  if (!m->combine_forced) m->combine = s.combine != 0 && m->combine_ok;
  if (!getenv("CFS_HIP_NT")) m->nt_stream = s.nt_stream != 0;
  *out = m.release();
  return 0;
}

int cfs_hip_sym_load(const char *path, const char *expected_tag, cfs_hip_sym_t *out) {
  if (out) *out = nullptr;
  if (!path || !out) return set_err(CFS_HIP_ERR_ARG, "null argument");
  std::string err;
  uint64_t fsize = 0;
  FILE *f = pf::open_plan(path, &fsize, err);
  if (!f) return set_err(CFS_HIP_ERR_FILE, err);
  struct Closer {
    FILE *f;
    ~Closer() { fclose(f); }
  } closer{f};
  std::unique_ptr<pf::Parsed> F(new pf::Parsed());
  if (pf::parse_file(f, fsize, *F, err)) return set_err(CFS_HIP_ERR_FILE, std::string(path) + ": " + err);
  if (expected_tag && strcmp(expected_tag, F->h.tag) != 0)
    return set_err(CFS_HIP_ERR_FILE, std::string(path) + ": tag mismatch: the file was saved with \"" + F->h.tag +
                                         "\", the caller expects \"" + expected_tag + "\"");
  const int rc = F->h.value_bytes == 8 ? sym_load<double>(f, path, *F, out) : sym_load<float>(f, path, *F, out);
  if (rc) *out = nullptr;
  return rc;
}

int cfs_hip_plan_file_check(const char *path, cfs_hip_plan_file_info *info) {
  if (!path || !info) return set_err(CFS_HIP_ERR_ARG, "null argument");
  memset(info, 0, sizeof *info);
  std::unique_ptr<pf::Parsed> F(new pf::Parsed());
  std::string err;
  if (pf::check_file(path, *F, err)) return set_err(CFS_HIP_ERR_FILE, err);
  const pf::Header &h = F->h;
  const pf::Scalars &s = h.s;
  info->format_version = (int)h.version, info->value_bytes = (int)h.value_bytes;
  info->n = (int)s.n, info->row_begin = (int)s.row_begin, info->row_end = (int)s.row_end;
  info->nranks = (int)s.nranks, info->rank = (int)s.rank, info->flags = (int)s.flags;
  info->ntiles = (int)s.ntiles, info->ngroups = (int)s.ngroups, info->block_threads = (int)s.block_threads;
  info->lds_slots = (int)s.lds_slots, info->has_value_map = (int)s.has_value_map, info->deterministic = (int)s.deterministic;
  info->device_built = (int)s.device_built, info->nsections = (int)h.nsections;
  info->nnz_low = s.nnz_low, info->nslices = s.nslices, info->halo_slots = s.nhalo, info->stream_len = s.stream_len;
  info->fold_rows = s.nfold, info->remote_vals = s.nsend, info->mirror_entries = s.mirror_entries;
  info->far_entries = s.far_entries, info->payload_bytes = (int64_t)h.payload_bytes, info->file_bytes = (int64_t)h.file_bytes;
  snprintf(info->tag, sizeof info->tag, "%s", h.tag);
  return 0;
}

// developer / test: the file checksum of a byte range, by the device kernel (p a 16-byte aligned device
// pointer) or by the host function (cfs_hip.h)
int cfs_hip_debug_checksum(const void *p, size_t bytes, int on_device, unsigned long long *out) {
  if (!out || (bytes && !p)) return set_err(CFS_HIP_ERR_ARG, "null argument");
  if (!on_device) {
    *out = pf::checksum(p, bytes);
    return 0;
  }
  int rc = ensure_init();
  if (rc) return rc;
  const cfs_rt::PtrInfo pi = cfs_rt::classify(p);
  if (bytes && !pi.device) return set_err(CFS_HIP_ERR_ARG, "not a device pointer");
  DeviceGuard g(pi.device ? pi.dev : -1);
  const void *ptr[1] = {p};
  uint64_t len[1] = {bytes}, sum[1] = {0};
  if ((rc = device_checksums(ptr, len, 1, sum, (hipStream_t)0))) return rc;
  *out = sum[0];
  return 0;
}

template <typename V>
static int plan_save(int n, const int *rowptr, const int *colind, const V *values, int nranks, int rank,
                     const int *row_splits, const cfs_hip_options *opt, const char *path, const char *tag) {
  if (!path) return set_err(CFS_HIP_ERR_ARG, "path is NULL");
  if (tag && strlen(tag) > (size_t)pf::kTagMax) return set_err(CFS_HIP_ERR_ARG, "tag longer than 255 bytes");
  if (n < 0 || !rowptr || (n > 0 && rowptr[n] > 0 && (!colind || !values)))
    return set_err(CFS_HIP_ERR_ARG, "null CSR array");
  if (nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !row_splits))
    return set_err(CFS_HIP_ERR_ARG, "bad rank / nranks / row_splits");
  SymPlan<V> P;
  const cfs_plan::Options po = to_opts(opt);
  if (!cfs_plan::build_plan<V>(n, rowptr, colind, values, nranks, rank, nranks > 1 ? row_splits : nullptr, po, P))
    return set_err(plan_error_code(P.error), P.error);
  pf::Extras x;
  x.flags = opt ? opt->flags : 0, x.num_cus = po.num_cus, x.nnz_caller = rowptr[n];
  x.combine = SymMatrix<V>::size_rule_combine(P), x.nt_stream = SymMatrix<V>::size_rule_nt(P);
  std::string err;
  if (!pf::save_plan(P, x, path, tag, err)) return set_err(CFS_HIP_ERR_FILE, err);
  return 0;
}
int cfs_hip_sym_plan_save_f64(int n, const int *rowptr, const int *colind, const double *values, int nranks, int rank,
                              const int *row_splits, const cfs_hip_options *opt, const char *path, const char *tag) {
  return plan_save<double>(n, rowptr, colind, values, nranks, rank, row_splits, opt, path, tag);
}
int cfs_hip_sym_plan_save_f32(int n, const int *rowptr, const int *colind, const float *values, int nranks, int rank,
                              const int *row_splits, const cfs_hip_options *opt, const char *path, const char *tag) {
  return plan_save<float>(n, rowptr, colind, values, nranks, rank, row_splits, opt, path, tag);
}

// ---- general CSR ------------------------------------------------------------
int cfs_hip_csr_create_f64(int nrows, int ncols, const int *rowptr, const int *colind,
                           const double *values, cfs_hip_csr_t *out) {
  return csr_create<double>(nrows, ncols, rowptr, colind, values, out);
}
int cfs_hip_csr_create_f32(int nrows, int ncols, const int *rowptr, const int *colind,
                           const float *values, cfs_hip_csr_t *out) {
  return csr_create<float>(nrows, ncols, rowptr, colind, values, out);
}

int cfs_hip_csr_spmv_async(cfs_hip_csr_t h, void *y, const void *x, void *stream) {
  if (!h || !y || !x) return set_err(CFS_HIP_ERR_ARG, "null argument");
  DeviceGuard g(h->device);
  if (!h->form_measured) {
    int rc = csr_choose_form(h, y, x, (hipStream_t)stream);
    if (rc) return rc;
  }
  return csr_launch(h, y, x, (hipStream_t)stream);
}
int cfs_hip_csr_kernel_form(cfs_hip_csr_t h, int *form, int *measured) {
  if (!h || !form) return set_err(CFS_HIP_ERR_ARG, "null argument");
  *form = h->block_form ? CFS_HIP_CSR_FORM_BLOCK : CFS_HIP_CSR_FORM_WAVE;
  if (measured) *measured = h->form_measured ? 1 : 0;
  return 0;
}

int cfs_hip_csr_stats(cfs_hip_csr_t h, int64_t *bytes_streamed, int64_t *narrow_nnz) {
  if (!h) return set_err(CFS_HIP_ERR_ARG, "null argument");
  const int64_t vb = h->value_bytes, nz = h->nnz;
  int64_t b = nz * vb + ((int64_t)h->nrows + 1) * 4;
  const int64_t nar = h->wide == 2 ? h->narrow_nnz : 0;
  if (h->block_form) b += nar * 2 + (nz - nar) * 4 + (int64_t)h->nblocks * (h->cbase.p ? 20 : 4);
  else b += nz * 4 + (int64_t)h->nchunks * 16;
  if (bytes_streamed) *bytes_streamed = b;
  if (narrow_nnz) *narrow_nnz = h->block_form && h->wide == 2 ? h->narrow_nnz : 0;
  return 0;
}

int cfs_hip_csr_debug_layout(cfs_hip_csr_t h, long long *words, int capacity_words) {
  if (!h || !words || capacity_words < CFS_HIP_CSR_LAYOUT_WORDS) return set_err(CFS_HIP_ERR_ARG, "bad argument");
  return csr_debug_layout(h, words);
}

int cfs_hip_csr_spmv(cfs_hip_csr_t h, void *y, const void *x) {
  if (!h || !y || !x) return set_err(CFS_HIP_ERR_ARG, "null argument");
  const size_t vb = (size_t)h->value_bytes;
  return run_staged(h->device, h->stage, (size_t)h->ncols * vb, (size_t)h->nrows * vb, y, x,
                    [&](void *yd, const void *xd, hipStream_t st) {
                      return cfs_hip_csr_spmv_async(h, yd, xd, (void *)st);
                    });
}

int cfs_hip_csr_destroy(cfs_hip_csr_t h) {
  delete h;
  return 0;
}

// ---- events -------------------------------------------------------------------
int cfs_hip_event_create(void **ev) {
  int rc = ensure_init();
  if (rc) return rc;
  hipEvent_t e;
  HIPCHK(hipEventCreate(&e));
  *ev = (void *)e;
  return 0;
}
int cfs_hip_event_record(void *ev, void *stream) {
  HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
  return 0;
}
int cfs_hip_event_elapsed_ms(void *start, void *stop, float *ms) {
  HIPCHK(hipEventSynchronize((hipEvent_t)stop));
  HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return 0;
}
int cfs_hip_event_destroy(void *ev) {
  HIPCHK(hipEventDestroy((hipEvent_t)ev));
  return 0;
}
